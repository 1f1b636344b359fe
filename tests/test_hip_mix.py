"""The batch-mixing kernels on the device (csrc/mix.hip) against the oracle of tests/mix_oracle.py.

Mixing is a selection: every comparison is ``torch.equal`` (float tensors as int32 words, so NaN payloads count) - there is no
tolerance anywhere in this file.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

SELECT_GEOMS = [(1, 2, 1, 1), (2, 3, 5, 7), (3, 21, 37, 53), (2, 64, 64, 64), (2, 2, 96, 130), (1, 3, 3, 300)]
APPLY_GEOMS = SELECT_GEOMS + [(1, 3, 7, 1), (2, 4, 64, 68)]
_ids = lambda g: "x".join(map(str, g))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(t, a):
    """A device tensor equals a numpy array bit for bit."""
    want = torch.from_numpy(np.ascontiguousarray(a))
    got = t.detach().cpu()
    if got.dtype == torch.float32:
        got, want = got.contiguous().view(torch.int32), want.view(torch.int32)
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def _labels(rng, B, C, H, W, ignore=True):
    lab = rng.integers(0, C, (B, H, W)).astype(np.int64)
    if ignore and H * W >= 8:
        lab[rng.random((B, H, W)) < 0.05] = 255
        lab[rng.random((B, H, W)) < 0.05] = -100
    return lab


def _offset_view(t):
    """The same values as a dense view at a storage offset of one element (4 or 8 bytes off every 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


def _path(ops):
    """Which apply kernel the last call took: 4 pixels per lane (16-byte accesses) or 1."""
    trace = ops.last_launches()
    assert trace.count("mix_apply<") == 1, trace
    return 4 if "mix_apply<4>" in trace else 1


# ------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("geom", SELECT_GEOMS, ids=_ids)
def test_class_select_equals_the_oracle(dev, geom):
    from weaklysuperviseddl_amd import ops
    B, C, H, W = geom
    rng = np.random.default_rng(sum(geom))
    seed_sets = [rng.integers(-2 ** 63, 2 ** 63 - 1, B), np.arange(B) - 1, np.full(B, -2 ** 63)]
    for k, seeds in enumerate(seed_sets):
        lab = _labels(rng, B, C, H, W)
        if k == 1:
            lab[0] = (255, -100)[B % 2]                                       # an image of ignore values only
        if k == 2 and H * W >= 4 * C:
            lab.reshape(B, -1)[:, :C] = np.arange(C)                           # every class present
        seeds = seeds.astype(np.int64)
        lab_dev, seeds_dev = _d(lab, dev), _d(seeds, dev)
        keep = lab_dev.clone()
        for cands in (None, (1,), tuple(range(0, C, 2))):
            sel, pres = ops.mix_class_select(lab_dev, C, seeds_dev, candidates=cands)
            want_sel, want_pres = O.class_select(lab, C, seeds, cands)
            assert _same(sel, want_sel) and _same(pres, want_pres), (geom, k, cands)
            if k == 2 and H * W >= 4 * C and cands is None:
                assert int(pres[0].item()) & O.MASK64 == (1 << C) - 1
        assert torch.equal(lab_dev, keep)
    # out= reuse over stale contents, and two calls identical
    out = {"sel": torch.full((B,), -1, dtype=torch.int64, device=dev), "present": torch.full((B,), -1, dtype=torch.int64, device=dev)}
    s1, p1 = ops.mix_class_select(lab_dev, C, seeds_dev, out=out)
    assert s1 is out["sel"] and p1 is out["present"] and _same(s1, want_sel if cands is None else O.class_select(lab, C, seeds)[0])
    s2, p2 = ops.mix_class_select(lab_dev, C, seeds_dev)
    assert torch.equal(s1, s2) and torch.equal(p1, p2)
    # a view at an odd storage offset, a non-dense map
    s3, p3 = ops.mix_class_select(_offset_view(lab_dev), C, _offset_view(seeds_dev))
    wide = torch.zeros(B, H, W + 3, dtype=torch.int64, device=dev)
    wide[:, :, :W] = lab_dev
    s4, p4 = ops.mix_class_select(wide[:, :, :W], C, seeds_dev)
    assert torch.equal(s3, s1) and torch.equal(p3, p1) and torch.equal(s4, s1) and torch.equal(p4, p1)


# ----------------------------------------------------------------------------------------------------------------- apply
def _partners(rng, B):
    """Self-partners, duplicates, -1 and B (both unmixed), and a random draw."""
    sets = [np.arange(B), np.zeros(B), np.full(B, -1), np.full(B, B), rng.integers(-1, B + 1, B), (np.arange(B) + 1) % B]
    return [s.astype(np.int32) for s in sets]


def _nan_sprinkle(rng, x):
    """NaNs with payloads, infinities and negative zeros, written as integer words."""
    w = x.view(np.uint32).reshape(-1)
    idx = rng.choice(w.size, size=max(1, w.size // 16), replace=False)
    w[idx] = rng.choice(np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x7FA0BEEF], dtype=np.uint32), size=idx.size)
    return x


def _case(rng, geom, i):
    B, C, H, W = geom
    Ci, Cs = (1, 3, 4)[i % 3], (2, 21, 64)[i % 3]
    img = _nan_sprinkle(rng, rng.standard_normal((B, Ci, H, W)).astype(F))
    lab = _labels(rng, B, 2, H, W) * 255
    pw = _nan_sprinkle(rng, rng.random((B, H, W)).astype(F))
    sc = _nan_sprinkle(rng, rng.standard_normal((B, Cs, H, W)).astype(F))
    return img, lab, pw, sc


def _source(rng, kind, geom, i, dev, ops):
    """The mask source of ``kind`` -> (keyword arguments for the oracle, the same for the device)."""
    B, C, H, W = geom
    if kind == "box":
        R = (1, 8, 3)[i % 3]
        y0, x0 = rng.integers(-5, H + 2, (B, R)), rng.integers(-5, W + 2, (B, R))
        boxes = np.stack([y0, x0, y0 + rng.integers(-2, H + 5, (B, R)), x0 + rng.integers(-2, W + 5, (B, R))], axis=-1).astype(np.int32)
        return dict(boxes=boxes), dict(boxes=_d(boxes, dev))
    if kind == "class":
        cls = _labels(rng, B, C, H, W)
        seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, B).astype(np.int64)
        sel, _ = O.class_select(cls, C, seeds)
        sel_dev, _ = ops.mix_class_select(_d(cls, dev), C, _d(seeds, dev))
        assert _same(sel_dev, sel)
        return dict(class_labels=cls, sel=sel), dict(class_labels=_d(cls, dev), sel=sel_dev)
    mask = (rng.random((B, H, W)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (B, H, W)).astype(np.uint8)
    return dict(mask=mask), dict(mask=_d(mask, dev))


def _check(res, want, names):
    for n in names:
        assert _same(getattr(res, n), want[n]), n


@pytest.mark.parametrize("geom", APPLY_GEOMS, ids=_ids)
@pytest.mark.parametrize("kind", ["box", "class", "mask"])
def test_mix_batch_equals_the_oracle(dev, kind, geom):
    """Each kind at each geometry: the vector path on dense aligned tensors where W % 4 == 0, the scalar path otherwise and on
    views at a storage offset of one element; every partner pattern; all tensors, the mask and the count; ``invert``."""
    from weaklysuperviseddl_amd import ops
    i = APPLY_GEOMS.index(geom)
    B, C, H, W = geom
    rng = np.random.default_rng(100 * i + len(kind))
    img, lab, pw, sc = _case(rng, geom, i)
    src_np, src_dev = _source(rng, kind, geom, i, dev, ops)
    if geom == (2, 4, 64, 68):
        # W a multiple of 4, sliced from a wider tensor: the row pitch breaks alignment - densified, as the other ops do
        def widen(a):
            t = torch.zeros(a.shape[:-1] + (W + 4,), dtype=torch.from_numpy(a).dtype, device=dev)
            t[..., :W] = _d(a, dev)
            v = t[..., :W]
            assert not v.is_contiguous()
            return v
    else:
        widen = lambda a: _d(a, dev)  # noqa: E731
    img_d, lab_d, pw_d, sc_d = widen(img), widen(lab), widen(pw), widen(sc)
    keep = [t.clone() for t in (img_d, lab_d, pw_d, sc_d)] + [v.clone() for v in src_dev.values()]
    ops.launch_trace(True)
    try:
        for k, partner in enumerate(_partners(rng, B)):
            invert = k % 2 == 1
            par_d = _d(partner, dev)
            ops.last_launches()
            # every tensor, the mask and the count
            res = ops.mix_batch(img_d, lab_d, par_d, kind=kind, invert=invert, pixel_weight=pw_d, scores=sc_d, want_mask=True,
                                want_count=True, **src_dev)
            assert _path(ops) == (4 if W % 4 == 0 else 1)
            want = O.mix_batch(img, lab, partner, kind=kind, invert=invert, pixel_weight=pw, scores=sc, **src_np)
            _check(res, want, ("images", "labels", "pixel_weight", "scores", "mask", "mixed_count"))
            if not ((partner >= 0) & (partner < B)).any():
                assert _same(res.images, img) and _same(res.labels, lab) and not res.mask.any() and not res.mixed_count.any()
            # images and labels alone
            res2 = ops.mix_batch(img_d, lab_d, par_d, kind=kind, invert=invert, **src_dev)
            _check(res2, want, ("images", "labels"))
            assert res2.pixel_weight is None and res2.scores is None and res2.mask is None and res2.mixed_count is None
        # views at a storage offset of one element take the scalar path and give the same bits; two calls identical
        ops.last_launches()
        res3 = ops.mix_batch(_offset_view(img_d.contiguous()), _offset_view(lab_d.contiguous()), par_d, kind=kind, invert=invert,
                             pixel_weight=_offset_view(pw_d.contiguous()), scores=_offset_view(sc_d.contiguous()), want_mask=True,
                             want_count=True, **{n: (_offset_view(v) if n != "sel" else v) for n, v in src_dev.items()})
        assert _path(ops) == 1
        for n in ("images", "labels", "pixel_weight", "scores", "mask", "mixed_count"):
            a, b = getattr(res3, n), getattr(res, n)
            assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), n
    finally:
        ops.launch_trace(False)
    for t, k0 in zip([img_d, lab_d, pw_d, sc_d] + list(src_dev.values()), keep):          # inputs untouched
        assert torch.equal(_bits(t) if t.dtype == torch.float32 else t, _bits(k0) if k0.dtype == torch.float32 else k0)


def test_boxes_at_the_edges(dev):
    """Empty boxes, the whole image, overlapping boxes, boxes partly and wholly outside, negative corners; R = 1 and 8."""
    from weaklysuperviseddl_amd import ops
    B, H, W = 3, 37, 53
    rng = np.random.default_rng(8)
    img = rng.standard_normal((B, 3, H, W)).astype(F)
    lab = rng.integers(0, 2, (B, H, W)).astype(np.int64)
    partner = np.array([1, 2, 0], dtype=np.int32)
    big = 2 ** 31 - 1
    named = {
        "empty": [0, 0, 0, 0], "empty_y": [5, 3, 5, 9], "reversed": [9, 9, 3, 3], "whole": [0, 0, H, W], "beyond": [-7, -9, H + 4, W + 11],
        "inner": [3, 4, 20, 30], "overlap": [10, 20, 30, 40], "corner": [-5, -5, 4, 6], "far_corner": [H - 3, W - 2, H + 9, W + 9],
        "outside": [H, 0, H + 5, W], "left_of": [0, -20, H, 0], "one_pixel": [H - 1, W - 1, H, W], "extreme": [-big - 1, -big - 1, big, big],
    }
    names = list(named)
    # R = 1: every named box alone, three items at a time
    for k in range(0, len(names), B):
        rows = [named[names[(k + j) % len(names)]] for j in range(B)]
        boxes = np.array(rows, dtype=np.int64).astype(np.int32).reshape(B, 1, 4)
        res = ops.mix_batch(_d(img, dev), _d(lab, dev), _d(partner, dev), kind="box", boxes=_d(boxes, dev), want_mask=True, want_count=True)
        want = O.mix_batch(img, lab, partner, kind="box", boxes=boxes)
        _check(res, want, ("images", "labels", "mask", "mixed_count"))
    counts = {n: int(O.mix_mask("box", [0], (1, H, W), boxes=np.array([[named[n]]], dtype=np.int64))[0].sum()) for n in names}
    assert counts["empty"] == counts["empty_y"] == counts["reversed"] == counts["outside"] == counts["left_of"] == 0
    assert counts["whole"] == counts["beyond"] == counts["extreme"] == H * W and counts["corner"] == 24 and counts["one_pixel"] == 1
    # R = 8: unions, with empty boxes among them
    for inv in (False, True):
        rows = [[named[n] for n in ("inner", "overlap", "empty", "corner", "far_corner", "outside", "one_pixel", "reversed")],
                [named["empty"]] * 8, [named["whole"]] + [named["inner"]] * 7]
        boxes = np.array(rows, dtype=np.int32)
        res = ops.mix_batch(_d(img, dev), _d(lab, dev), _d(partner, dev), kind="box", boxes=_d(boxes, dev), invert=inv, want_mask=True,
                            want_count=True)
        want = O.mix_batch(img, lab, partner, kind="box", boxes=boxes, invert=inv)
        _check(res, want, ("images", "labels", "mask", "mixed_count"))
        assert want["mixed_count"].tolist()[1:] == ([H * W, 0] if inv else [0, H * W])


def test_out_reuse_refusals_and_determinism(dev):
    from weaklysuperviseddl_amd import ops
    B, Ci, H, W = 2, 3, 16, 24
    rng = np.random.default_rng(3)
    img, lab = _d(rng.standard_normal((B, Ci, H, W)).astype(F), dev), _d(rng.integers(0, 2, (B, H, W)).astype(np.int64), dev)
    pw = torch.rand(B, H, W, device=dev)
    par = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    mask = (torch.rand(B, H, W, device=dev) < 0.5).to(torch.uint8)
    out = {"images": torch.full_like(img, 7.0), "labels": torch.full_like(lab, 7), "pixel_weight": torch.full_like(pw, 7.0),
           "mask": torch.full_like(mask, 7), "mixed_count": torch.full((B,), 7, dtype=torch.int64, device=dev)}
    res = ops.mix_batch(img, lab, par, kind="mask", mask=mask, pixel_weight=pw, want_mask=True, want_count=True, out=out)
    assert all(getattr(res, k) is out[k] for k in out) and res.scores is None
    again = ops.mix_batch(img, lab, par, kind="mask", mask=mask, pixel_weight=pw, want_mask=True, want_count=True)
    for k in out:
        a, b = getattr(res, k), getattr(again, k)
        assert a is not b and torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), k
    assert torch.equal(res.mask, (mask != 0).to(torch.uint8)) and torch.equal(res.mixed_count, mask.flatten(1).sum(1))
    assert torch.equal(res.images, torch.where(mask[:, None] != 0, img.flip(0), img))
    # an output over an input is refused on the host: item b reads item partner[b]
    for kw, what in ((dict(out={"images": img}), "images"), (dict(out={"labels": lab}), "labels"),
                     (dict(pixel_weight=pw, out={"pixel_weight": pw}), "pixel_weight"),
                     (dict(want_mask=True, out={"mask": mask}), "mask")):
        with pytest.raises(ops.WsdlError, match=f"shares memory with {what}"):
            ops.mix_batch(img, lab, par, kind="mask", mask=mask, **kw)
    big = torch.zeros(2 * img.numel(), device=dev)
    with pytest.raises(ops.WsdlError, match="shares memory with images"):
        ops.mix_batch(big[:img.numel()].view_as(img), lab, par, kind="mask", mask=mask, out={"images": big[8:8 + img.numel()].view_as(img)})
    # the library refuses it too, and a kind without its source
    t = (ops._MixTensor * 1)()
    t[0].src, t[0].dst, t[0].channels, t[0].elem_bytes = img.data_ptr(), img.data_ptr() + 64, Ci, 4
    import ctypes as C
    rc = ops.lib().wsdl_mix_apply(C.cast(t, C.c_void_p), 1, par.data_ptr(), 2, None, 0, None, None, mask.data_ptr(), 0, B, H, W, None, None, None)
    assert rc != 0 and "overlaps" in ops.lib().wsdl_last_error().decode()
    with pytest.raises(ops.WsdlError, match="needs sel"):
        ops.mix_batch(img, lab, par, kind="class", class_labels=lab)


# ------------------------------------------------------------------------------------------------------------ launch plan
def test_a_plan_replays_the_selection_and_the_mix_on_new_contents(dev):
    from weaklysuperviseddl_amd import ops, plan
    B, C, Ci, H, W = 3, 5, 3, 40, 52

    def contents(seed):
        r = np.random.default_rng(seed)
        return dict(img=r.standard_normal((B, Ci, H, W)).astype(F), lab=_labels(r, B, C, H, W), pw=r.random((B, H, W)).astype(F),
                    sc=r.standard_normal((B, C, H, W)).astype(F), par=r.permutation(B).astype(np.int32),
                    seeds=r.integers(-2 ** 63, 2 ** 63 - 1, B).astype(np.int64))
    a, b = contents(1), contents(2)
    b["par"][0] = -1
    t = {k: _d(v, dev) for k, v in a.items()}
    sel_out = {k: torch.empty(B, dtype=torch.int64, device=dev) for k in ("sel", "present")}
    out = {"images": torch.empty_like(t["img"]), "labels": torch.empty_like(t["lab"]), "pixel_weight": torch.empty_like(t["pw"]),
           "scores": torch.empty_like(t["sc"]), "mask": torch.empty(B, H, W, dtype=torch.uint8, device=dev),
           "mixed_count": torch.empty(B, dtype=torch.int64, device=dev)}

    def call(t, sel_out, out):
        sel, _ = ops.mix_class_select(t["lab"], C, t["seeds"], out=sel_out)
        return ops.mix_batch(t["img"], t["lab"], t["par"], kind="class", class_labels=t["lab"], sel=sel, pixel_weight=t["pw"],
                             scores=t["sc"], want_mask=True, want_count=True, out=out)
    p, _ = plan.record(call, t, sel_out, out)
    want = ops.mix_launches("class", select=True, want_count=True)
    assert want == {"kernels": 3, "memsets": 2} and p.stats["kernels"] == want["kernels"] and p.stats["memsets"] == want["memsets"]

    def check(c):
        sel, pres = O.class_select(c["lab"], C, c["seeds"])
        assert _same(sel_out["sel"], sel) and _same(sel_out["present"], pres)
        w = O.mix_batch(c["img"], c["lab"], c["par"], kind="class", class_labels=c["lab"], sel=sel, pixel_weight=c["pw"], scores=c["sc"])
        for k in out:
            assert _same(out[k], w[k]), k
    check(a)
    for k, v in b.items():                                  # new contents, partners and seeds at the recorded addresses
        t[k].copy_(_d(v, dev))
    for v in list(out.values()) + list(sel_out.values()):
        v.fill_(5)
    p.replay()
    check(b)
    # bit-identical to eager calls on the same contents
    eager = call({k: _d(v, dev) for k, v in b.items()}, None, None)
    for k in out:
        e = getattr(eager, k)
        assert torch.equal(_bits(out[k]) if e.dtype == torch.float32 else out[k], _bits(e) if e.dtype == torch.float32 else e), k
    p2, _ = plan.record(lambda: ops.mix_batch(t["img"], t["lab"], t["par"], kind="box",
                                              boxes=torch.zeros(B, 2, 4, dtype=torch.int32, device=dev), out={k: out[k] for k in ("images", "labels")}))
    assert p2.stats["kernels"] == ops.mix_launches("box")["kernels"] == 1 and p2.stats["memsets"] == 0


# ------------------------------------------------------------------------------------------------------- the training step
def _batch(B, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, S, S, generator=g)
    masks = (torch.rand(B, S, S, generator=g) > 0.5).long() * 255
    return img.to(dev), masks.to(dev)


def _deeplab(dev, with_ema=False):
    from weaklysuperviseddl_amd import ema as E
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    torch.manual_seed(0)
    model = build_segmentation_model().to(dev).train()
    opt = make_optimizer(model, lr=1e-4)
    avg = E.FlatEMA(opt, model, build_segmentation_model().to(dev), decay=0.5, warmup=False) if with_ema else None
    return model, opt, avg


def _planned(opt):
    return next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)


def _mix_params(kind, n, B, S, dev, seed, prob=1.0):
    from weaklysuperviseddl_amd.augment import Mix
    mix = Mix(kind, prob=prob, boxes=2)
    return mix, mix.epoch_params(n, B, (S, S), dev, torch.Generator().manual_seed(seed))


def _state(opt, avg):
    return opt.flat_param.clone(), (None if avg is None else avg.ema_param.clone())


def test_unmixed_steps_equal_the_mean_teacher_step_and_train_step(dev):
    """Every partner -1: with an EMA the step equals ``train_step_mean_teacher(mode="replace")`` bit for bit - losses, parameters,
    teacher - and with ``ema=None`` it equals ``train_step``."""
    from weaklysuperviseddl_amd.augment import Mix
    from weaklysuperviseddl_amd.TraditionalModel import train_step, train_step_mean_teacher, train_step_mixed
    B, S = 2, 64
    batches = [_batch(B, S, dev, s) for s in (1, 2)]
    mix, params = _mix_params("cutmix", 2, B, S, dev, 3, prob=0.0)
    assert (params["partner"] == -1).all()

    def run(with_ema, mixed):
        model, opt, avg = _deeplab(dev, with_ema=with_ema)
        torch.manual_seed(1234)
        losses = []
        for i, (img, m) in enumerate(batches):
            if mixed:
                losses.append(float(train_step_mixed(model, avg, opt, img, m, mix, Mix.step_params(params, i), tau=0.5)))
            elif with_ema:
                losses.append(float(train_step_mean_teacher(model, avg, opt, img, m, tau=0.5, mode="replace")))
            else:
                losses.append(float(train_step(model, opt, img, m)))
        return (losses,) + _state(opt, avg)
    for with_ema in (True, False):
        a, b = run(with_ema, True), run(with_ema, False)
        assert all(np.isfinite(a[0])) and a[0] == b[0] and torch.equal(a[1], b[1]), with_ema
        if with_ema:
            assert torch.equal(a[2], b[2])


@pytest.mark.parametrize("config", ["cutmix", "classmix_conf", "cutmix_consistency", "copy_paste_no_teacher"])
def test_a_mixed_step_equals_its_composition_from_the_public_ops(dev, config):
    from weaklysuperviseddl_amd import nn as wnn, ops
    from weaklysuperviseddl_amd.augment import Mix
    from weaklysuperviseddl_amd.TraditionalModel import train_step, train_step_mixed
    B, S = 2, 64
    batches = [_batch(B, S, dev, s) for s in (1, 2)]
    kind = config.split("_")[0] if not config.startswith("copy") else "copy_paste"
    mix, params = _mix_params(kind, 2, B, S, dev, 5)
    by_conf, with_cons, with_ema = config == "classmix_conf", config == "cutmix_consistency", not config.endswith("no_teacher")

    def run(composed):
        model, opt, avg = _deeplab(dev, with_ema=with_ema)
        crit = wnn.CrossEntropyLoss() if by_conf else None
        cons = wnn.ConsistencyLoss(kind="kl", tau=0.5, lam=1.0).to(dev) if with_cons else None
        torch.manual_seed(1234)
        losses, mixed_px = [], 0
        for i, (img, m) in enumerate(batches):
            par = Mix.step_params(params, i)
            if not composed:
                losses.append(float(train_step_mixed(model, avg, opt, img, m, mix, par, crit, tau=0.5, weight_by_conf=by_conf,
                                                     consistency=cons)))
                continue
            labels, logits, conf = m.long(), None, None
            if with_ema:
                with torch.no_grad():
                    logits = avg.teacher(img)["out"]
                labels = ops.clamp_max_labels(labels, 1)
                if by_conf:
                    labels, conf = ops.teacher_targets(logits, labels, 0.5, "replace", conf=True)
                else:
                    labels = ops.teacher_targets(logits, labels, 0.5, "replace")
            kw = dict(pixel_weight=conf, scores=logits if with_cons else None, want_count=True)
            if kind == "cutmix":
                res = ops.mix_batch(img, labels, par["partner"], kind="box", boxes=par["boxes"], **kw)
            else:
                cls = labels if with_ema else ops.clamp_max_labels(labels, 1)
                sel, _ = ops.mix_class_select(cls, 2, par["seeds"], candidates=mix.candidates)
                res = ops.mix_batch(img, labels, par["partner"], kind="class", class_labels=cls, sel=sel, **kw)
            mixed_px += int(res.mixed_count.sum())
            if by_conf:
                crit.set_pixel_weight(res.pixel_weight)
            if with_cons:
                cons.set_teacher(res.scores)
            losses.append(float(train_step(model, opt, res.images, res.labels, extra_loss=cons, criterion=crit)))
        return (losses, mixed_px) + _state(opt, avg)
    a, b = run(True), run(False)
    # something was mixed; two boxes of at most half the image each never cover all of it (a class set may: a teacher that
    # predicts one class everywhere hands the whole partner over)
    assert 0 < a[1] and (kind != "cutmix" or a[1] < 2 * B * S * S)
    assert all(np.isfinite(a[0])) and a[0] == b[0] and torch.equal(a[2], b[2])
    if with_ema:
        assert torch.equal(a[3], b[3])


def test_the_planned_mixed_step_equals_the_eager_one_and_the_defaults_are_unchanged(dev):
    """Five mixed steps with ``plan.PLAN_STEP`` on and off give the same bits, the marks show one record (third call) and then
    replays; ``train_step`` and ``train_step_mean_teacher`` give the same bits before and after the feature has been used."""
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.augment import Mix
    from weaklysuperviseddl_amd.TraditionalModel import train_step, train_step_mean_teacher, train_step_mixed
    B, S = 2, 64
    batches = [_batch(B, S, dev, s) for s in (1, 2, 3)]

    def defaults():
        model, opt, avg = _deeplab(dev, with_ema=True)
        torch.manual_seed(99)
        out = [float(train_step(model, opt, *batches[0])), float(train_step_mean_teacher(model, avg, opt, *batches[1], tau=0.5))]
        return (out,) + _state(opt, avg)
    before = defaults()
    mix, params = _mix_params("classmix", 5, B, S, dev, 9)

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            model, opt, avg = _deeplab(dev, with_ema=True)
            torch.manual_seed(1234)
            losses, marks = [], []
            for i in range(5):
                img, m = batches[i % 3]
                losses.append(float(train_step_mixed(model, avg, opt, img, m, mix, Mix.step_params(params, i), tau=0.5)))
                st = _planned(opt)
                marks.append(None if st is None else (st.records, st.replays, st.disabled))
            return (losses, marks) + _state(opt, avg)
        finally:
            plan.PLAN_STEP[0] = old
    e, p = run(False), run(True)
    assert all(np.isfinite(p[0])) and e[0] == p[0] and torch.equal(e[2], p[2]) and torch.equal(e[3], p[3])
    assert all(m[2] is None for m in p[1]), p[1]
    assert [m[:2] for m in p[1]] == [(0, 0), (0, 0), (1, 0), (1, 1), (1, 2)], p[1]
    after = defaults()
    assert before[0] == after[0] and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
