"""csrc/augment.hip on the device: ``ops.augment_batch`` against the numpy restatement of its contract
(tests/augment_oracle.py) at the smallest shapes at which it can go wrong, the 64-bit offsets at a Pet-sized source, the two
device loaders with an augmentation, and ``train_step`` on batches that carry the padding label."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as O  # noqa: E402
from conftest import report_line  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W = 4, 13, 17
OUT = (16, 24)                  # another size than the source, a fraction of the 128-column tile
IDX = [2, 0, 2]
PAD_VALUE, PAD_LABEL = 0.25, -100
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rows():
    """name -> (parameter row, output size)."""
    from weaklysuperviseddl_amd.augment import affine_row
    src = (H, W)
    r = lambda *a, **k: tuple(affine_row(*a, **k).tolist())          # noqa: E731
    return {
        "identity": (O.IDENTITY, src),                                # out = src: 13 rows, no multiple of the 4-row tile
        "flip": (r(0.0, src, OUT, flip=True), OUT),
        "rot30": (r(30.0, src, OUT), OUT),
        "scale0.25": (r(0.0, src, OUT, scale=0.25), OUT),            # ignore: 1/16 of the output is valid; reflect: several periods
        "scale2": (r(0.0, src, OUT, scale=2.0), OUT),
        "far": ((1, 0, 1000, 0, 1, 0, 1, 0), OUT),
        "gain_bias": (r(0.0, src, OUT, gain=1.2, bias=-0.1), OUT),
    }


ROW_NAMES = ["identity", "flip", "rot30", "scale0.25", "scale2", "far", "gain_bias"]


@pytest.fixture(scope="module")
def data():
    """The sources (made once, never written) and a cache of oracle results."""
    rng = np.random.default_rng(17)
    lut = ((np.arange(256, dtype=np.float32) / np.float32(255))[None] - np.array([[0.485], [0.456], [0.406]], np.float32)) \
        / np.array([[0.229], [0.224], [0.225]], np.float32)
    d = {
        "f32": rng.standard_normal((N, 3, H, W)).astype(np.float32),
        "u8": rng.integers(0, 256, (N, 3, H, W), dtype=np.uint8),
        "lut": np.ascontiguousarray(lut.astype(np.float32)),
        "labels": rng.integers(0, 256, (N, H, W), dtype=np.uint8),
        "rows": _rows(),
        "worst": {},
    }
    d["M"] = {"f32": float(np.abs(d["f32"]).max()), "u8": float(np.abs(d["lut"]).max())}
    return d


def _run(dev, images, labels, idx, params, out_hw, fill, lut=None, label_lut=None):
    from weaklysuperviseddl_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    gi, gl = ops.augment_batch(t(images), t(labels), torch.tensor(idx, dtype=torch.int64, device=dev),
                               torch.tensor(params, dtype=torch.float32, device=dev), out_hw, lut=t(lut), label_lut=t(label_lut),
                               fill=fill, pad_value=PAD_VALUE, pad_label=PAD_LABEL)
    assert gi.dtype == torch.float32 and gl.dtype == torch.int64
    return gi.cpu().numpy(), gl.cpu().numpy()


def _check(name, got, want, params, M):
    """labels equal; |gpu - oracle| <= 32 * 2^-24 * (|gain| * M + |bias|) per item.  Derived, not measured: float32 roundings
    of magnitude at most 2M through the three lerps give about 20 M 2^-24, gain and bias add about two more at
    |gain| M + |bias|; rounded up to 32.  Returns the worst ratio to the bound."""
    (gi, gl), (wi, wl) = got, want
    assert gi.shape == wi.shape and gl.shape == wl.shape
    assert np.array_equal(gl, wl), f"{name}: {(gl != wl).sum()} of {wl.size} labels differ"
    worst = 0.0
    for b, row in enumerate(np.asarray(params, dtype=np.float32)):
        bound = 32 * EPS * (abs(float(row[6])) * M + abs(float(row[7])))
        err = float(np.abs(gi[b].astype(np.float64) - wi[b]).max())
        worst = max(worst, err / bound)
        assert err <= bound, f"{name}: item {b}: |gpu - oracle| = {err:.3e} > {bound:.3e}"
    return worst


@pytest.mark.parametrize("row", ROW_NAMES)
@pytest.mark.parametrize("fill", ["ignore", "reflect"])
@pytest.mark.parametrize("source", ["f32", "u8"])
def test_parity_matrix(dev, data, source, fill, row):
    params, out_hw = data["rows"][row]
    params = [params] * len(IDX)
    lut = data["lut"] if source == "u8" else None
    want = O.augment_batch(data[source], data["labels"], IDX, params, out_hw, lut=lut, fill=fill, pad_value=PAD_VALUE,
                           pad_label=PAD_LABEL)
    got = _run(dev, data[source], data["labels"], IDX, params, out_hw, fill, lut=lut)
    valid = float((want[1] != PAD_LABEL).mean())
    if row == "far" and fill == "ignore":
        assert valid == 0.0 and (got[0] == np.float32(PAD_VALUE)).all()
    if row == "scale0.25" and fill == "ignore":
        assert 0.03 < valid < 0.1, valid
    if fill == "reflect":
        assert valid == 1.0
    if row == "identity":          # exact, not only within the bound
        src = data["f32"] if source == "f32" else np.stack([data["lut"][c][data["u8"][:, c]] for c in range(3)], axis=1)
        assert np.array_equal(got[0], src[IDX]) and np.array_equal(got[1], data["labels"][IDX].astype(np.int64))
    data["worst"][(source, fill, row)] = _check(f"{source}/{fill}/{row}", got, want, params, data["M"][source])


def test_parity_report(dev, data):
    """(after the matrix) the worst observed ratio to the derived bound, for the record."""
    if data["worst"]:
        k = max(data["worst"], key=data["worst"].get)
        report_line(f"augment_batch: worst |gpu - oracle| / bound over {len(data['worst'])} cases = {data['worst'][k]:.3f} at {k}")


def test_items_with_their_own_rows(dev, data):
    """Seven items, seven different rows, repeated and unordered source rows: parameters and the gather are per item."""
    names = [n for n in ROW_NAMES if n != "identity"] + ["rot30"]
    params = [data["rows"][n][0] for n in names]
    idx = [3, 1, 1, 0, 2, 3, 0]
    for fill in ("ignore", "reflect"):
        want = O.augment_batch(data["f32"], data["labels"], idx, params, OUT, fill=fill, pad_value=PAD_VALUE, pad_label=PAD_LABEL)
        got = _run(dev, data["f32"], data["labels"], idx, params, OUT, fill)
        _check("own rows/" + fill, got, want, params, data["M"]["f32"])
    # ... and an item's result does not depend on the batch it is in
    one = _run(dev, data["f32"], data["labels"], idx[2:3], params[2:3], OUT, "reflect")
    assert np.array_equal(one[0][0], got[0][2]) and np.array_equal(one[1][0], got[1][2])


@pytest.mark.parametrize("out_hw", [(16, 23), (33, 70), (5, 130), (1, 1)])
def test_odd_output_sizes(dev, data, out_hw):
    """Sizes that are no multiple of the 128 x 4 tile or of a wave's 64 columns: odd widths, a width just past one tile
    (130), a last tile row whose second row of threads and whose threads' second pixel fall off the end (33, 5, 1)."""
    from weaklysuperviseddl_amd.augment import affine_row
    params = [tuple(affine_row(-20.0, (H, W), out_hw, scale=0.8, gain=0.9, bias=0.05).tolist())] * len(IDX)
    for fill in ("ignore", "reflect"):
        want = O.augment_batch(data["u8"], data["labels"], IDX, params, out_hw, lut=data["lut"], fill=fill,
                               pad_value=PAD_VALUE, pad_label=PAD_LABEL)
        got = _run(dev, data["u8"], data["labels"], IDX, params, out_hw, fill, lut=data["lut"])
        _check(f"odd {out_hw}/{fill}", got, want, params, data["M"]["u8"])


def test_one_channel(dev, data):
    params = [data["rows"]["rot30"][0]] * len(IDX)
    for source, lut in (("f32", None), ("u8", data["lut"][1:2])):
        src = np.ascontiguousarray(data[source][:, 1:2])
        want = O.augment_batch(src, data["labels"], IDX, params, OUT, lut=lut, fill="ignore", pad_value=PAD_VALUE,
                               pad_label=PAD_LABEL)
        got = _run(dev, src, data["labels"], IDX, params, OUT, "ignore", lut=lut)
        assert got[0].shape == (3, 1) + OUT
        M = data["M"]["f32"] if lut is None else float(np.abs(lut).max())
        _check("C=1/" + source, got, want, params, M)


def test_label_table(dev, data):
    table = ((np.arange(256) * 7) % 5 - 1).astype(np.int64)
    params = [data["rows"]["rot30"][0]] * len(IDX)
    want = O.augment_batch(data["f32"], data["labels"], IDX, params, OUT, label_lut=table, fill="ignore", pad_value=PAD_VALUE,
                           pad_label=PAD_LABEL)
    got = _run(dev, data["f32"], data["labels"], IDX, params, OUT, "ignore", label_lut=table)
    _check("label table", got, want, params, data["M"]["f32"])
    assert set(np.unique(got[1])) <= set(table.tolist()) | {PAD_LABEL}


def test_index_outside_the_source_is_all_padding(dev, data):
    """The kernel never reads through a bad index: the item comes out as padding, its neighbours are untouched."""
    params = [O.IDENTITY] * 3
    gi, gl = _run(dev, data["f32"], data["labels"], [1, N, -1], params, (H, W), "reflect")
    assert np.array_equal(gi[0], data["f32"][1]) and np.array_equal(gl[0], data["labels"][1].astype(np.int64))
    assert (gi[1:] == np.float32(PAD_VALUE)).all() and (gl[1:] == PAD_LABEL).all()


def test_bad_arguments(dev, data):
    from weaklysuperviseddl_amd import WsdlError, ops
    t = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    img, lab = t(data["f32"]), t(data["labels"])
    idx = torch.tensor(IDX, device=dev)
    params = torch.tensor([O.IDENTITY] * 3, dtype=torch.float32, device=dev)
    with pytest.raises(WsdlError, match="lut"):
        ops.augment_batch(t(data["u8"]), lab, idx, params)
    with pytest.raises(WsdlError, match="C = 2"):
        ops.augment_batch(img[:, :2].contiguous(), lab, idx, params)
    with pytest.raises(WsdlError, match="params"):
        ops.augment_batch(img, lab, idx, params[:2])
    with pytest.raises(WsdlError, match="fill"):
        ops.augment_batch(img, lab, idx, params, fill="wrap")
    with pytest.raises(WsdlError, match="labels"):
        ops.augment_batch(img, lab[:, :, :5].contiguous(), idx, params)
    with pytest.raises(WsdlError, match="out_size"):
        ops.augment_batch(img, lab, idx, params, (0, 4))
    with pytest.raises(WsdlError, match="no CPU fallback"):
        ops.augment_batch(img, lab, idx.cpu(), params)


def test_offsets_past_2_to_the_31(dev):
    """A Pet-sized uint8 source (2.26 GB): item 14999 starts 2.26e9 bytes in; with 32-bit offsets it would come from elsewhere."""
    from weaklysuperviseddl_amd import ops
    n = 15000
    images = torch.empty(n, 3, 224, 224, dtype=torch.uint8, device=dev)
    labels = torch.empty(n, 224, 224, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(4)
    first = torch.randint(0, 256, (2, 3, 224, 224), generator=g).to(torch.uint8).to(dev)
    first_l = torch.randint(1, 4, (2, 224, 224), generator=g).to(torch.uint8).to(dev)
    images[0], images[n - 1] = first[0], first[1]
    labels[0], labels[n - 1] = first_l[0], first_l[1]
    table = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).to(dev)
    lut = table.view(1, 256).repeat(3, 1).contiguous()
    idx = torch.tensor([n - 1, 0], device=dev)
    params = torch.tensor([O.IDENTITY] * 2, dtype=torch.float32, device=dev)
    gi, gl = ops.augment_batch(images, labels, idx, params, lut=lut)
    assert torch.equal(gi, table[first.flip(0).to(torch.int32)])
    assert torch.equal(gl, first_l.flip(0).to(torch.int64))
    del images, labels
    torch.cuda.empty_cache()


# ---- the loaders -----------------------------------------------------------------------------------------------------------
def _pet(dev, n=10, side=40, seed=0):
    """A DevicePetDataset from tensors: what the decode pass leaves, without the decode."""
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DevicePetDataset, _to_float_table
    g = torch.Generator().manual_seed(seed)
    ds = DevicePetDataset.__new__(DevicePetDataset)
    ds.device = dev
    ds.images = torch.randint(0, 256, (n, 3, side, side), generator=g).to(torch.uint8).to(dev)
    ds.trimaps = torch.randint(1, 4, (n, side, side), generator=g).to(torch.uint8).to(dev)
    ds.categories = torch.zeros(n, dtype=torch.int64, device=dev)
    ds._table = _to_float_table().to(dev)
    return ds


def _pseudo(dev, n=10, side=40, seed=1):
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import InMemoryPseudoDataset
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(n, 3, side, side, generator=g).to(dev)
    masks = ((torch.rand(n, side, side, generator=g) > 0.5).to(torch.uint8) * 255).to(dev)
    return InMemoryPseudoDataset(images, masks)


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def test_loader_identity(dev):
    from weaklysuperviseddl_amd.augment import Augment
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DeviceLoader
    ds = _pet(dev)
    for kw in (dict(), dict(shuffle=True, drop_single=True), dict(indices=[7, 1, 8, 2, 9])):
        gens = [torch.Generator().manual_seed(3) for _ in range(2)]
        plain = list(DeviceLoader(ds, 4, generator=gens[0], **kw))
        ident = list(DeviceLoader(ds, 4, generator=gens[1], augment=Augment.identity(), **kw))
        assert len(plain) == (2 if "indices" in kw else 3) and _same(plain, ident)
    assert plain[0][0].dtype == torch.float32 and plain[0][1].dtype == torch.int64

    ps = _pseudo(dev)
    plain = list(ps.batches(4, shuffle=False))
    ident = list(ps.batches(4, shuffle=False, augment=Augment.identity()))
    assert len(plain) == 3 and _same(plain, ident)
    assert set(torch.cat([b[1].flatten() for b in ident]).unique().tolist()) == {0, 255}          # 255 stays 255
    gens = [torch.Generator().manual_seed(8) for _ in range(2)]
    assert _same(list(ps.batches(4, generator=gens[0], limit=2)),
                 list(ps.batches(4, generator=gens[1], limit=2, augment=Augment.identity())))


def test_loader_determinism_and_flip(dev):
    from weaklysuperviseddl_amd.augment import Augment
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DeviceLoader
    ds, ps = _pet(dev), _pseudo(dev)
    aug = Augment(scale=(0.5, 2.0), rotate=30.0, hflip=0.5, brightness=0.1, contrast=0.2)
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(21)
        loader = DeviceLoader(ds, 4, shuffle=True, generator=g, augment=aug)
        runs.append((list(loader), list(loader), list(ps.batches(4, generator=g, augment=aug))))
    for a, b in zip(runs[0], runs[1]):
        assert _same(a, b)                                      # same seed: bit for bit, epoch by epoch
    g = torch.Generator().manual_seed(21)
    still = DeviceLoader(ds, 4, shuffle=False, generator=g, augment=aug)
    e1, e2 = list(still), list(still)
    assert not any(torch.equal(x[0], y[0]) for x, y in zip(e1, e2))          # the same items, new parameters every epoch
    labels = torch.cat([b[1].flatten() for b in e1]).unique().tolist()
    assert set(labels) <= {0, 1, -100} and -100 in labels and 1 in labels
    # reflect pads nothing
    refl = list(DeviceLoader(ds, 4, generator=torch.Generator().manual_seed(21),
                             augment=Augment(scale=(0.5, 2.0), rotate=30.0, fill="reflect")))
    assert set(torch.cat([b[1].flatten() for b in refl]).unique().tolist()) == {0, 1}

    flip = Augment(hflip=1.0)
    for plain, mirrored in ((list(DeviceLoader(ds, 4)), list(DeviceLoader(ds, 4, augment=flip))),
                            (list(ps.batches(4, shuffle=False)), list(ps.batches(4, shuffle=False, augment=flip)))):
        assert len(plain) == len(mirrored) == 3
        for p, m in zip(plain, mirrored):
            assert torch.equal(m[0], p[0].flip(-1)) and torch.equal(m[1], p[1].flip(-1))
    # another output size: the batches take it
    big = next(iter(DeviceLoader(ds, 4, augment=Augment(rotate=10.0, out_size=(48, 56)))))
    assert tuple(big[0].shape) == (4, 3, 48, 56) and tuple(big[1].shape) == (4, 48, 56)


# ---- train_step on batches that carry the padding label ----------------------------------------------------------------------
def _model_and_opt(dev, seed=0):
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    torch.manual_seed(seed)
    model = build_segmentation_model().to(dev).train()
    return model, make_optimizer(model, lr=1e-4)


def _copy_into(twin, model):
    """``twin`` becomes a copy of ``model`` as it is now: parameters, BatchNorm statistics, the dropout modules' seed and
    call counter."""
    from weaklysuperviseddl_amd import nn as wnn
    twin.load_state_dict(model.state_dict())
    for a, b in zip(model.modules(), twin.modules()):
        if isinstance(a, wnn.Dropout):
            b._seed = a._seed
            b._counter = None if a._counter is None else a._counter.clone()


@pytest.mark.parametrize("loss_fn", ["lovasz_hinge", "cross_entropy"])
def test_train_step_ignores_the_padding(dev, loss_fn):
    """The loss a step returns is the loss of the logits of a copy of the model taken before the step, with the padded border
    left out - on eager calls and, from the third call on, through the planned step."""
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    g = torch.Generator().manual_seed(6)
    images = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    labels = (torch.rand(2, 64, 64, generator=g) > 0.5).long()
    labels[:, :9], labels[:, -5:], labels[:, :, :7], labels[:, :, -11:] = -100, -100, -100, -100
    labels = labels.to(dev)
    model, opt = _model_and_opt(dev)
    twin, _twin_opt = _model_and_opt(dev)
    if loss_fn == "lovasz_hinge":
        kw = dict(loss_fn="lovasz_hinge", ignore_label=-100)
        expect = lambda out: ops.lovasz_hinge(out, labels, ignore=-100)          # noqa: E731
    else:
        kw = dict(loss_fn="cross_entropy")
        expect = lambda out: ops.cross_entropy(out, labels)                      # noqa: E731
    for call in range(5):
        _copy_into(twin, model)
        torch.manual_seed(100 + call)          # (the first forward of a Dropout module draws its host seed here)
        want = expect(twin(images)["out"]).detach()
        torch.manual_seed(100 + call)
        got = train_step(model, opt, images, labels, **kw)
        assert torch.equal(got, want), (loss_fn, call, float(got), float(want))
        assert math.isfinite(float(got))
    st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
    assert st is not None
    if loss_fn == "cross_entropy":
        assert st.disabled is None and st.replays >= 1, (st.disabled, st.replays)
    # the padding is really left out: the same step with the border counted as class 0 gives another loss
    if loss_fn == "lovasz_hinge":
        _copy_into(twin, model)
        torch.manual_seed(7)
        out = twin(images)["out"].detach()
        assert not torch.equal(ops.lovasz_hinge(out, labels, ignore=-100), ops.lovasz_hinge(out, labels.clamp(min=0)))
