"""The oracle of the batch-mixing kernels (tests/mix_oracle.py) and the host side of the feature - no device needed.

  * the oracle's class selection against a brute-force sort of ``(key, c)`` on hand-made cases;
  * the frequency of the selection rule: seeds 0..4095, five present sets, every class selected at a frequency within 0.04 of
    k / n (one standard deviation of a fair draw over 4096 seeds is 0.008);
  * ``augment.Mix.draw``: determinism, what it leaves undrawn, boxes, partners, the share of unmixed items;
  * the refusals of ``ops.check_mix_options`` / ``ops.check_mix_select_options`` that need no device.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_oracle as O  # noqa: E402


def _brute(labels_i, num_classes, seed, candidates=None):
    """present and selected classes by sorting (key, c)."""
    cands = set(range(num_classes)) if candidates is None else set(candidates)
    present = [c for c in range(num_classes) if c in cands and (labels_i == c).any()]
    order = sorted(present, key=lambda c: (O.key(seed, c), c))
    return sorted(order[:(len(present) + 1) // 2]), present


def _map_with(classes, extra=(), shape=(6, 11)):
    vals = list(classes) + list(extra)
    lab = np.resize(np.array(vals if vals else [255], dtype=np.int64), shape[0] * shape[1]).reshape(shape)
    return lab


# ------------------------------------------------------------------------------------------------------------ the selection
def test_fmix_is_the_splitmix64_finaliser():
    # splitmix64 from state 0: the first output is fmix(GOLDEN) (the published test vector of the generator)
    assert O.fmix(O.GOLDEN) == 0xE220A8397B1DCDAF
    assert O.key(0, 0) == O.fmix(O.GOLDEN) and O.key(-1, 0) == O.fmix((O.GOLDEN - 1) & O.MASK64)


@pytest.mark.parametrize("classes", [(), (4,), (0, 1), (1, 2, 5), tuple(range(64))], ids=lambda c: f"n{len(c)}")
def test_selection_against_a_brute_force_sort(classes):
    """n = 0, 1, 2, 3, 64 present classes, with ignore values sprinkled in, over positive, negative and huge seeds."""
    lab = _map_with(classes, extra=(255, -100, 64, -1), shape=(9, 17))
    for seed in (0, 1, -1, 12345, -(2 ** 63), 2 ** 63 - 1, 2 ** 40 + 7):
        sel, pres = O.class_select(lab[None], 64, [seed])
        want_sel, want_pres = _brute(lab, 64, seed)
        assert want_pres == sorted(classes)
        assert int(pres[0]) & O.MASK64 == O.word(want_pres) and int(sel[0]) & O.MASK64 == O.word(want_sel), (classes, seed)
        assert len(want_sel) == (len(classes) + 1) // 2


def test_selection_with_candidates_and_ignore_only_maps():
    lab = _map_with((0, 1, 3, 7), extra=(255,))
    for seed in range(20):
        for cands in ((1,), (0, 1), (3, 7, 9), (9,), ()):
            sel, pres = O.class_select(lab[None], 21, [seed], candidates=cands)
            want_sel, want_pres = _brute(lab, 21, seed, cands)
            assert int(pres[0]) == O.word(want_pres) and int(sel[0]) == O.word(want_sel), (seed, cands)
        # copy-paste: the foreground whenever it is present
        assert int(O.class_select(lab[None], 21, [seed], candidates=(1,))[0][0]) == 0b10
    # a class >= num_classes is not present, labels that are all ignore give the empty sets
    assert O.present_classes(_map_with((0, 5)), 3) == [0]
    for fill in (255, -100):
        sel, pres = O.class_select(np.full((2, 4, 5), fill, dtype=np.int64), 64, [3, 4])
        assert not sel.any() and not pres.any()


def test_every_class_is_selected_at_its_fair_frequency():
    seeds = range(4096)
    for present in ([0, 1], [0, 3, 7, 20], [1, 2, 5], list(range(21)), [5, 63]):
        n, k = len(present), (len(present) + 1) // 2
        hits = dict.fromkeys(present, 0)
        for s in seeds:
            chosen = O.select_classes(present, s)
            assert len(chosen) == k
            for c in chosen:
                hits[c] += 1
        for c in present:
            assert abs(hits[c] / len(seeds) - k / n) <= 0.04, (present, c, hits[c] / len(seeds), k / n)


def test_oracle_masks_and_apply_on_a_hand_made_case():
    B, H, W = 3, 4, 5
    img = np.arange(B * 2 * H * W, dtype=np.float32).reshape(B, 2, H, W)
    lab = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W)
    partner = np.array([1, -1, 0], dtype=np.int32)
    boxes = np.array([[[1, 1, 3, 4]], [[0, 0, 4, 5]], [[-5, -5, 1, 99]]], dtype=np.int32)
    r = O.mix_batch(img, lab, partner, kind="box", boxes=boxes)
    assert r["mixed_count"].tolist() == [6, 0, 5] and r["mask"][0, 1:3, 1:4].all() and r["mask"][0].sum() == 6
    assert np.array_equal(r["images"][0, :, 1:3, 1:4], img[1, :, 1:3, 1:4]) and np.array_equal(r["images"][1], img[1])
    assert np.array_equal(r["labels"][2, 0], lab[0, 0]) and np.array_equal(r["labels"][2, 1:], lab[2, 1:])
    inv = O.mix_batch(img, lab, partner, kind="box", boxes=boxes, invert=True)
    assert inv["mixed_count"].tolist() == [H * W - 6, 0, H * W - 5]             # unmixed stays unmixed
    # class: item 0 takes partner 1's pixels of the classes of sel[1]
    cls = np.array([[0, 1, 2, 255, -100]] * H, dtype=np.int64)[None].repeat(B, 0)
    sel = np.array([0, 0b101, 0], dtype=np.int64)
    rc = O.mix_batch(img, lab, partner, kind="class", class_labels=cls, sel=sel)
    assert rc["mask"][0].tolist() == [[1, 0, 1, 0, 0]] * H and not rc["mask"][2].any()
    # NaN payloads travel bit for bit
    x = np.array([0x7FC00001, 0x7F800000, 0xFFC12345, 0x80000000], dtype=np.uint32).view(np.float32).reshape(2, 1, 1, 2)
    rn = O.mix_batch(x, np.zeros((2, 1, 2), np.int64), np.array([1, 0], np.int32), kind="mask", mask=np.ones((2, 1, 2), np.uint8))
    assert np.array_equal(rn["images"].view(np.uint32), x.view(np.uint32)[::-1])


# --------------------------------------------------------------------------------------------------------------- Mix.draw
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_draw_is_deterministic_and_shaped():
    from weaklysuperviseddl_amd.augment import Mix
    for kind in ("cutmix", "classmix", "copy_paste"):
        m = Mix(kind, prob=0.7, boxes=3, partner="permute")
        a, b = m.draw(5, 4, (33, 47), _gen(3)), m.draw(5, 4, (33, 47), _gen(3))
        assert all(torch.equal(a[k], b[k]) for k in a) and sorted(a) == ["boxes", "partner", "seeds"]
        assert a["partner"].dtype == torch.int32 and tuple(a["partner"].shape) == (5, 4)
        assert a["boxes"].dtype == torch.int32 and tuple(a["boxes"].shape) == (5, 4, 3, 4)
        assert a["seeds"].dtype == torch.int64 and tuple(a["seeds"].shape) == (5, 4)
        c = m.draw(5, 4, (33, 47), _gen(4))
        assert not all(torch.equal(a[k], c[k]) for k in a)
    cm = Mix("classmix").draw(64, 4, (8, 8), _gen(0))["seeds"]
    assert (cm < 0).any() and (cm > 0).any() and cm.unique().numel() == cm.numel()       # the whole int64 range
    assert not Mix("copy_paste").draw(3, 4, (8, 8), _gen(0))["seeds"].any()             # one candidate: no seed matters
    assert Mix("copy_paste").candidates == (1,) and Mix("classmix").candidates is None
    step = Mix.step_params(Mix("cutmix").draw(3, 2, (8, 8), _gen(0)), 1)
    assert tuple(step["partner"].shape) == (2,) and tuple(step["boxes"].shape) == (2, 1, 4)


def test_draw_leaves_the_generator_alone_where_nothing_varies():
    from weaklysuperviseddl_amd.augment import Mix
    g = _gen(11)
    state = g.get_state().clone()
    # prob = 1 (and 0), one-point ranges: only positions could vary - and copy-paste / B <= 2 under "roll" draw nothing at all
    for m, B in ((Mix("copy_paste", prob=1.0), 1), (Mix("copy_paste", prob=1.0), 2), (Mix("copy_paste", prob=0.0), 2),
                 (Mix("copy_paste", prob=1.0, partner="permute"), 1)):
        out = m.draw(4, B, (16, 16), g)
        assert torch.equal(g.get_state(), state), (m.kind, B)
        want = -1 if m.prob == 0.0 else (0 if B == 1 else None)
        if want is not None:
            assert (out["partner"] == want).all()
    assert Mix("copy_paste").draw(4, 2, (16, 16), g)["partner"].tolist() == [[1, 0]] * 4
    # a component that cannot vary draws nothing: the later components see the same stream
    full = Mix("cutmix", area=(0.25, 0.5), aspect=(1.0, 1.0)).draw(3, 1, (32, 32), _gen(5))
    g2 = _gen(5)
    frac = 0.25 + 0.25 * torch.rand(3, 1, 1, generator=g2, dtype=torch.float64)
    uy = torch.rand(3, 1, 1, generator=g2, dtype=torch.float64)
    side = torch.sqrt(frac * 1024).round().to(torch.int64)
    assert torch.equal(full["boxes"][..., 2] - full["boxes"][..., 0], side.to(torch.int32))
    assert torch.equal(full["boxes"][..., 0].to(torch.int64), torch.minimum((uy * (32 - side + 1)).floor().to(torch.int64), 32 - side))
    fixed = Mix("cutmix", area=(0.25, 0.25), aspect=(1.0, 1.0)).draw(3, 1, (32, 32), _gen(5))
    assert ((fixed["boxes"][..., 2] - fixed["boxes"][..., 0]) == 16).all() and ((fixed["boxes"][..., 3] - fixed["boxes"][..., 1]) == 16).all()
    g3 = _gen(5)
    uy3 = torch.rand(3, 1, 1, generator=g3, dtype=torch.float64)                   # the first draw is already the row position
    assert torch.equal(fixed["boxes"][..., 0].to(torch.int64), (uy3 * 17).floor().to(torch.int64).clamp(max=16))


def test_boxes_lie_inside_the_image_with_the_drawn_area():
    from weaklysuperviseddl_amd.augment import Mix
    H = W = 64
    lo, hi = 0.25, 0.5
    bx = Mix("cutmix", area=(lo, hi), aspect=(0.5, 2.0)).draw(500, 4, (H, W), _gen(1))["boxes"].reshape(-1, 4).to(torch.int64)
    assert bx.shape[0] == 2000
    y0, x0, y1, x1 = bx.unbind(1)
    assert (y0 >= 0).all() and (x0 >= 0).all() and (y1 <= H).all() and (x1 <= W).all() and (y1 > y0).all() and (x1 > x0).all()
    area = (y1 - y0) * (x1 - x0)
    assert (area >= lo * H * W - (H + W)).all() and (area <= hi * H * W + (H + W)).all(), (int(area.min()), int(area.max()))
    assert y0.unique().numel() > 8 and x0.unique().numel() > 8 and area.unique().numel() > 50
    # extreme requests are clamped into the image: still inside, still non-empty
    for hw, kw in (((5, 300), dict(area=(0.9, 1.0), aspect=(0.01, 100.0))), ((1, 1), {}), ((7, 3), dict(area=(1e-6, 1e-5)))):
        b = Mix("cutmix", boxes=8, **kw).draw(50, 3, hw, _gen(2))["boxes"].reshape(-1, 4)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= hw[0]).all() and (b[:, 3] <= hw[1]).all()
        assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()


def test_partners_and_the_unmixed_share():
    from weaklysuperviseddl_amd.augment import Mix
    for B in (2, 3, 8):
        p = Mix("cutmix", partner="roll").draw(200, B, (8, 8), _gen(B))["partner"]
        item = torch.arange(B, dtype=torch.int32)[None]
        assert (p != item).all() and (p >= 0).all() and (p < B).all()
        shift = (p - item) % B
        assert (shift == shift[:, :1]).all() and shift[:, 0].unique().numel() == B - 1           # one shift per batch, all of them
    p = Mix("cutmix", partner="permute").draw(200, 6, (8, 8), _gen(9))["partner"]
    assert (p.sort(dim=1).values == torch.arange(6, dtype=torch.int32)[None]).all() and p.unique(dim=0).shape[0] > 100
    for partner in ("roll", "permute"):
        p = Mix("classmix", prob=0.5, partner=partner).draw(512, 8, (8, 8), _gen(21))["partner"]
        assert p.numel() == 4096 and abs(float((p == -1).float().mean()) - 0.5) <= 0.04
        assert ((p == -1) | ((p >= 0) & (p < 8))).all()
    assert (Mix("cutmix", prob=0.0).draw(3, 4, (8, 8), _gen(0))["partner"] == -1).all()
    with pytest.raises(ValueError, match="kind"):
        Mix("mixup")
    with pytest.raises(ValueError, match="partner"):
        Mix(partner="shuffle")
    with pytest.raises(ValueError, match="boxes"):
        Mix(boxes=9)
    with pytest.raises(ValueError, match="prob"):
        Mix(prob=1.5)
    with pytest.raises(ValueError, match="area"):
        Mix(area=(0.5, 1.5))


# -------------------------------------------------------------------------------------------------------------- refusals
def _args(B=2, Ci=3, H=4, W=6):
    return torch.zeros(B, Ci, H, W), torch.zeros(B, H, W, dtype=torch.int64), torch.zeros(B, dtype=torch.int32)


def test_check_mix_options_refuses_by_name_without_a_device():
    from weaklysuperviseddl_amd import ops
    img, lab, par = _args()
    B, H, W = lab.shape
    boxes = torch.zeros(B, 1, 4, dtype=torch.int32)
    sel = torch.zeros(B, dtype=torch.int64)
    msk = torch.zeros(B, H, W, dtype=torch.uint8)

    def bad(match, *a, **kw):
        with pytest.raises(ops.WsdlError, match=match):
            ops.check_mix_options(*a, **kw)
    bad("kind", img, lab, par, kind="cut", boxes=boxes)
    bad("images must be torch.float32", img.double(), lab, par, kind="box", boxes=boxes)
    bad("images must be a tensor of rank 4", img[0], lab, par, kind="box", boxes=boxes)
    bad("labels must be torch.int64", img, lab.int(), par, kind="box", boxes=boxes)
    bad("labels .* must be", img, lab[:, :-1], par, kind="box", boxes=boxes)
    bad("partner must be torch.int32", img, lab, par.long(), kind="box", boxes=boxes)
    bad("partner .* must be", img, lab, torch.zeros(B + 1, dtype=torch.int32), kind="box", boxes=boxes)
    bad("partner must be a tensor of rank 1", img, lab, par[:, None], kind="box", boxes=boxes)
    bad("empty dimension", img[:, :, :0], lab[:, :0], par, kind="box", boxes=boxes)
    bad("needs boxes", img, lab, par, kind="box")
    bad("R = 9", img, lab, par, kind="box", boxes=torch.zeros(B, 9, 4, dtype=torch.int32))
    bad("boxes .* must be", img, lab, par, kind="box", boxes=torch.zeros(B, 2, 3, dtype=torch.int32))
    bad("boxes must be torch.int32", img, lab, par, kind="box", boxes=boxes.long())
    bad("needs sel", img, lab, par, kind="class", class_labels=lab)
    bad("needs class_labels", img, lab, par, kind="class", sel=sel)
    bad("sel must be torch.int64", img, lab, par, kind="class", class_labels=lab, sel=sel.int())
    bad("needs mask", img, lab, par, kind="mask")
    bad("mask must be torch.uint8", img, lab, par, kind="mask", mask=msk.bool())
    bad("boxes belongs to kind='box'", img, lab, par, kind="mask", mask=msk, boxes=boxes)
    bad("C = 65", img, lab, par, kind="box", boxes=boxes, scores=torch.zeros(B, 65, H, W))
    bad("scores .* must be", img, lab, par, kind="box", boxes=boxes, scores=torch.zeros(B, 2, H, W + 1))
    bad("pixel_weight must be torch.float32", img, lab, par, kind="box", boxes=boxes, pixel_weight=torch.zeros(B, H, W).double())
    bad("invert", img, lab, par, kind="box", boxes=boxes, invert=1)
    bad("side lengths", torch.zeros(1, 1, 1, 16385), torch.zeros(1, 1, 16385, dtype=torch.int64), par[:1], kind="box", boxes=boxes[:1])
    # out: a dict of dense tensors of the results' shapes that share no memory with an input or with each other
    bad("out must be a dict", img, lab, par, kind="box", boxes=boxes, out=img)
    bad("out must be a dict", img, lab, par, kind="box", boxes=boxes, out={"image": img})
    bad(r"out\['images'\] shares memory with images", img, lab, par, kind="box", boxes=boxes, out={"images": img})
    bad(r"out\['labels'\] shares memory with labels", img, lab, par, kind="box", boxes=boxes, out={"labels": lab})
    wide = torch.zeros(2 * B, 3, H, W)
    bad(r"out\['images'\] shares memory with images", wide[:B], lab, par, kind="box", boxes=boxes, out={"images": wide[1:B + 1]})
    bad(r"out\['mask'\] shares memory with mask", img, lab, par, kind="mask", mask=msk, want_mask=True, out={"mask": msk})
    both = torch.zeros(B, 3, H, W)
    bad(r"out\['scores'\] shares memory with out\['images'\]", img, lab, par, kind="box", boxes=boxes, scores=torch.zeros(B, 3, H, W),
        out={"images": both, "scores": both})
    bad("does not produce", img, lab, par, kind="box", boxes=boxes, out={"mask": msk.clone()})
    bad(r"out\['images'\] must be a dense", img, lab, par, kind="box", boxes=boxes, out={"images": torch.zeros(B, 3, H, W + 1)})
    bad(r"out\['mixed_count'\] must be a dense", img, lab, par, kind="box", boxes=boxes, want_count=True,
        out={"mixed_count": torch.zeros(B, dtype=torch.int32)})
    # everything in order: the place is asked last - no CPU fallback
    bad("device tensor", img, lab, par, kind="box", boxes=boxes)
    with pytest.raises(ops.WsdlError, match="device tensor"):
        ops.mix_batch(img, lab, par, kind="mask", mask=msk)


def test_check_mix_select_options_and_mix_launches():
    from weaklysuperviseddl_amd import ops
    lab, seeds = torch.zeros(2, 4, 6, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)

    def bad(match, *a, **kw):
        with pytest.raises(ops.WsdlError, match=match):
            ops.check_mix_select_options(*a, **kw)
    bad("num_classes 65", lab, 65, seeds)
    bad("num_classes 0", lab, 0, seeds)
    bad("num_classes 2.0", lab, 2.0, seeds)
    bad("class_labels must be torch.int64", lab.int(), 2, seeds)
    bad("class_labels must be a tensor of rank 3", lab[0], 2, seeds)
    bad("seeds must be torch.int64", lab, 2, seeds.int())
    bad("seeds .* must be", lab, 2, seeds[:1])
    bad("candidates", lab, 2, seeds, candidates=(2,))
    bad("candidates", lab, 2, seeds, candidates=(-1,))
    bad("candidates", lab, 2, seeds, candidates=1)
    bad(r"out\['sel'\] shares memory with seeds", lab, 2, seeds, out={"sel": seeds})
    both = torch.zeros(2, dtype=torch.int64)
    bad(r"shares memory with out\['sel'\]", lab, 2, seeds, out={"sel": both, "present": both})
    bad("device tensor", lab, 2, seeds)
    with pytest.raises(ops.WsdlError, match="device tensor"):
        ops.mix_class_select(lab, 2, seeds)
    assert ops.mix_launches("box") == {"kernels": 1, "memsets": 0} == ops.mix_launches("mask")
    assert ops.mix_launches("class", want_count=True) == {"kernels": 1, "memsets": 1}
    assert ops.mix_launches("class", select=True, want_count=True) == {"kernels": 3, "memsets": 2}
    with pytest.raises(ops.WsdlError, match="select"):
        ops.mix_launches("box", select=True)
    with pytest.raises(ops.WsdlError, match="kind"):
        ops.mix_launches("cutmix")


def test_the_abi_refuses_bad_geometry_without_a_device():
    """Argument validation is host-side: a bad call returns an error before any launch."""
    import ctypes as C
    from weaklysuperviseddl_amd import _lib, ops
    L = _lib.lib()
    buf = (C.c_longlong * 64)()
    p = C.addressof(buf)
    assert L.wsdl_mix_class_select(p, p, 1, 65, 4, 4, 1, p, p + 64, None) != 0 and "C = 65" in L.wsdl_last_error().decode()
    assert L.wsdl_mix_class_select(p, p, 0, 2, 4, 4, 1, p, p + 64, None) != 0
    assert L.wsdl_mix_class_select(p, p, 1, 2, 4, 4, 1, p, p, None) != 0
    assert L.wsdl_mix_class_select(None, p, 1, 2, 4, 4, 1, p, p + 64, None) != 0 and "null" in L.wsdl_last_error().decode()
    t = (ops._MixTensor * 1)()
    t[0].src, t[0].dst, t[0].channels, t[0].elem_bytes = p, p + 256, 1, 4
    tp = C.cast(t, C.c_void_p)
    assert L.wsdl_mix_apply(tp, 1, p, 0, p, 9, None, None, None, 0, 1, 2, 2, None, None, None) != 0 and "R = 9" in L.wsdl_last_error().decode()
    assert L.wsdl_mix_apply(tp, 1, p, 3, p, 1, None, None, None, 0, 1, 2, 2, None, None, None) != 0 and "kind" in L.wsdl_last_error().decode()
    assert L.wsdl_mix_apply(tp, 5, p, 0, p, 1, None, None, None, 0, 1, 2, 2, None, None, None) != 0
    assert L.wsdl_mix_apply(tp, 1, p, 1, None, 0, None, None, None, 0, 1, 2, 2, None, None, None) != 0
    assert L.wsdl_mix_apply(tp, 1, p, 0, p + 128, 1, None, None, None, 0, 1, 2, 20000, None, None, None) != 0
    t[0].dst = p + 8                                                # the output over the input: refused, nothing launched
    assert L.wsdl_mix_apply(tp, 1, p + 384, 0, p + 448, 1, None, None, None, 0, 1, 2, 2, None, None, None) != 0
    assert "overlaps" in L.wsdl_last_error().decode()
