"""Joint image / label augmentation, host side (no GPU): the numpy oracle of csrc/augment.hip reproduces the exact cases of
the contract, ``augment.Augment`` draws what it documents, the product path refuses host tensors and a loader without an
augmentation touches nothing new."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as O  # noqa: E402

from weaklysuperviseddl_amd.augment import Augment, IDENTITY_ROW, affine_row  # noqa: E402

H, W = 13, 17
PAD_VALUE, PAD_LABEL = -7.5, -100
FILLS = ("ignore", "reflect")


@pytest.fixture(scope="module")
def source():
    rng = np.random.default_rng(5)
    return rng.standard_normal((3, H, W)).astype(np.float32), rng.integers(0, 256, (H, W), dtype=np.uint8)


def run(source, row, out_hw, fill):
    img, lab = source
    return O.augment_one(img, lab, row, out_hw, fill, PAD_VALUE, PAD_LABEL)


@pytest.mark.parametrize("fill", FILLS)
def test_oracle_identity_reproduces_the_input(source, fill):
    out, lab = run(source, O.IDENTITY, (H, W), fill)
    assert np.array_equal(out, source[0].astype(np.float64)) and np.array_equal(lab, source[1].astype(np.int64))


@pytest.mark.parametrize("fill", FILLS)
def test_oracle_flip(source, fill):
    out, lab = run(source, (-1, 0, W, 0, 1, 0, 1, 0), (H, W), fill)
    assert np.array_equal(out, source[0][..., ::-1].astype(np.float64))
    assert np.array_equal(lab, source[1][:, ::-1].astype(np.int64))


def test_oracle_translation_ignore(source):
    """xs = ox + 3, ys = oy - 2: the shifted slice, padding elsewhere."""
    out, lab = run(source, (1, 0, 3, 0, 1, -2, 1, 0), (H, W), "ignore")
    want = np.full((3, H, W), PAD_VALUE, dtype=np.float64)
    want_l = np.full((H, W), PAD_LABEL, dtype=np.int64)
    want[:, 2:, :W - 3] = source[0][:, :H - 2, 3:]
    want_l[2:, :W - 3] = source[1][:H - 2, 3:]
    assert np.array_equal(out, want) and np.array_equal(lab, want_l)


def test_oracle_translation_reflect(source):
    """The same translation with fill='reflect': numpy's symmetric padding, shifted."""
    out, lab = run(source, (1, 0, 3, 0, 1, -2, 1, 0), (H, W), "reflect")
    padded = np.pad(source[0], ((0, 0), (2, 0), (0, 3)), mode="symmetric")
    padded_l = np.pad(source[1], ((2, 0), (0, 3)), mode="symmetric")
    assert np.array_equal(out, padded[:, :H, 3:].astype(np.float64))
    assert np.array_equal(lab, padded_l[:H, 3:].astype(np.int64))


@pytest.mark.parametrize("fill", FILLS)
def test_oracle_quarter_turn(source, fill):
    """xs = v, ys = 13 - u on a (17, 13) output: the transposed source, flipped."""
    out, lab = run(source, (0, 1, 0, -1, 0, 13, 1, 0), (W, H), fill)
    assert np.array_equal(out, source[0].transpose(0, 2, 1)[..., ::-1].astype(np.float64))
    assert np.array_equal(lab, source[1].T[:, ::-1].astype(np.int64))


def test_oracle_far_translation_is_all_padding(source):
    out, lab = run(source, (1, 0, 1000, 0, 1, 0, 1, 0), (H, W), "ignore")
    assert (out == PAD_VALUE).all() and (lab == PAD_LABEL).all()
    # reflect never pads: 1000 = 29 periods of 34 + 14, so column ox reads position (14 + ox) of [source | mirrored source]
    out_r, lab_r = run(source, (1, 0, 1000, 0, 1, 0, 1, 0), (H, W), "reflect")
    cols = [(c if c < W else 2 * W - 1 - c) for c in ((ox + 1000) % (2 * W) for ox in range(W))]
    assert np.array_equal(out_r, source[0][..., cols].astype(np.float64)) and np.array_equal(lab_r, source[1][:, cols].astype(np.int64))


def test_oracle_gain_bias_and_label_table(source):
    lut = (np.arange(256) % 3).astype(np.int64)
    out, lab = O.augment_one(source[0], source[1], (1, 0, 0, 0, 1, 0, 1.25, -0.5), (H, W), "ignore", 0.0, -100, lut)
    assert np.array_equal(out, 1.25 * source[0].astype(np.float64) - 0.5) and np.array_equal(lab, lut[source[1]])


# ---- Augment.draw --------------------------------------------------------------------------------------------------------
def test_identity_row():
    a = Augment.identity()
    rows = a.draw(5, (H, W), (H, W))
    assert rows.dtype == torch.float32 and rows.device.type == "cpu" and tuple(rows.shape) == (5, 8)
    assert all(tuple(r.tolist()) == IDENTITY_ROW for r in rows)
    assert not torch.signbit(rows).any()
    assert tuple(affine_row(0.0, (H, W)).tolist()) == IDENTITY_ROW
    # the identity consumes nothing from the generator: a loader's shuffling is what it was
    g = torch.Generator().manual_seed(3)
    before = g.get_state().clone()
    a.draw(5, (H, W), (H, W), generator=g)
    assert torch.equal(g.get_state(), before)


def test_draw_is_deterministic_and_moves_on():
    a = Augment(scale=(0.5, 2.0), rotate=30.0, hflip=0.5, brightness=0.1, contrast=0.2)
    r1 = a.draw(64, (224, 224), (224, 224), torch.Generator().manual_seed(11))
    g = torch.Generator().manual_seed(11)
    r2 = a.draw(64, (224, 224), (224, 224), g)
    r3 = a.draw(64, (224, 224), (224, 224), g)
    assert torch.equal(r1, r2) and not torch.equal(r2, r3)


def _compose64(s, angle, flip, src_hw, out_hw):
    """An independent float64 composition with 3x3 matrices: out -> centred -> rotate -> flip -> 1 / scale -> source."""
    (Hs, Ws), (Ho, Wo) = src_hw, out_hw
    t = math.radians(angle)
    centre_out = np.array([[1, 0, -Wo / 2], [0, 1, -Ho / 2], [0, 0, 1]], dtype=np.float64)
    rot = np.array([[math.cos(t), -math.sin(t), 0], [math.sin(t), math.cos(t), 0], [0, 0, 1]], dtype=np.float64)
    flp = np.diag([-1.0 if flip else 1.0, 1.0, 1.0])
    zoom = np.diag([Ws / Wo / s, Hs / Ho / s, 1.0])
    centre_src = np.array([[1, 0, Ws / 2], [0, 1, Hs / 2], [0, 0, 1]], dtype=np.float64)
    return centre_src @ zoom @ flp @ rot @ centre_out


@pytest.mark.parametrize("src_hw,out_hw", [((224, 224), (224, 224)), ((13, 17), (16, 24))])
def test_draw_ranges_and_matrix(src_hw, out_hw):
    a = Augment(scale=(0.5, 2.0), rotate=30.0, hflip=0.5, brightness=0.1, contrast=0.2)
    g = torch.Generator().manual_seed(2)
    sample = a.sample(200, g)
    assert ((sample["scale"] >= 0.5) & (sample["scale"] <= 2.0)).all()
    assert (sample["angle"].abs() <= 30.0).all()
    assert ((sample["gain"] >= 0.8) & (sample["gain"] <= 1.2)).all()
    assert (sample["bias"].abs() <= 0.1).all()
    assert set(sample["flip"].tolist()) == {0.0, 1.0}
    assert sample["scale"].std() > 0.2 and sample["angle"].std() > 5           # really spread over the range
    rows = a.compose(sample, src_hw, out_hw)
    # draw() is sample() then compose() on the same generator stream
    assert torch.equal(rows, a.draw(200, src_hw, out_hw, torch.Generator().manual_seed(2)))
    for i in range(200):
        M = _compose64(sample["scale"][i].item(), sample["angle"][i].item(), sample["flip"][i].item() == 1.0, src_hw, out_hw)
        want = np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 0], M[1, 1], M[1, 2], sample["gain"][i].item(),
                         sample["bias"][i].item()], dtype=np.float64)
        got = rows[i].numpy().astype(np.float64)
        # one cast to float32 of a float64 value that two orders of composition agree on to a few ulp of float64
        assert np.allclose(got, want, rtol=2.0 ** -23, atol=2.0 ** -23 * max(src_hw)), (i, got, want)


def test_scale_is_magnification():
    """scale 0.5 shrinks the content to half the output: the output's corners read a source point half a side OUTSIDE."""
    row = affine_row(0.0, (100, 100), scale=0.5).tolist()
    assert row[0] == 2.0 and row[4] == 2.0 and row[2] == -50.0 and row[5] == -50.0
    row = affine_row(0.0, (100, 100), scale=2.0).tolist()
    assert row[0] == 0.5 and row[2] == 25.0


def test_hflip_one_always_flips():
    rows = Augment(hflip=1.0).draw(32, (H, W), (H, W), torch.Generator().manual_seed(0))
    assert all(tuple(r.tolist()) == (-1.0, 0.0, float(W), 0.0, 1.0, 0.0, 1.0, 0.0) for r in rows)


def test_bad_arguments():
    for kw in (dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)), dict(rotate=-1.0), dict(hflip=1.5), dict(fill="wrap")):
        with pytest.raises(ValueError):
            Augment(**kw)


# ---- the product path ----------------------------------------------------------------------------------------------------
def test_augment_batch_refuses_host_tensors():
    from weaklysuperviseddl_amd import WsdlError, ops
    images = torch.zeros(2, 3, 4, 4)
    labels = torch.zeros(2, 4, 4, dtype=torch.uint8)
    idx = torch.tensor([1, 0])
    params = torch.tensor([IDENTITY_ROW, IDENTITY_ROW])
    with pytest.raises(WsdlError, match="no CPU fallback"):
        ops.augment_batch(images, labels, idx, params)
    ds_images = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    with pytest.raises(WsdlError, match="no CPU fallback"):
        ops.augment_batch(ds_images, labels, idx, params, lut=torch.zeros(3, 256))


def test_library_refuses_bad_geometry_on_the_host():
    """wsdl_augment_batch validates before it touches a device: with pointers that are never dereferenced."""
    from weaklysuperviseddl_amd import _lib
    lib = _lib.lib()
    ok = dict(src=8, u8=0, lut=None, lab=8, llut=None, idx=8, params=8, N=4, C=3, H=13, W=17, B=3, oh=16, ow=24, fill=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.wsdl_augment_batch(a["src"], a["u8"], a["lut"], a["lab"], a["llut"], a["idx"], a["params"], a["N"], a["C"],
                                      a["H"], a["W"], a["B"], a["oh"], a["ow"], a["fill"], 0.0, -100, 8, 8, None)

    for bad in (dict(C=2), dict(C=4), dict(H=0), dict(W=16385), dict(oh=0), dict(ow=16385), dict(fill=2), dict(N=0), dict(B=0),
                dict(u8=1), dict(src=None), dict(idx=None), dict(params=None), dict(lab=None)):
        assert call(**bad) != 0, bad
        assert b"augment_batch" in lib.wsdl_last_error()


class _Recorder:
    """Stands in for an Augment: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"augment.{name} touched")


def test_loaders_without_augment_touch_nothing_new(monkeypatch):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DeviceLoader, DevicePetDataset, _to_float_table
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import InMemoryPseudoDataset

    def boom(*a, **k):
        raise AssertionError("ops.augment_batch called")
    monkeypatch.setattr(ops, "augment_batch", boom)
    saved = sys.modules.pop("weaklysuperviseddl_amd.augment")
    try:
        g = torch.Generator().manual_seed(0)
        images = torch.randn(5, 3, 8, 8, generator=g)
        masks = (torch.rand(5, 8, 8, generator=g) > 0.5).to(torch.uint8) * 255
        ds = InMemoryPseudoDataset(images, masks)
        got = list(ds.batches(2, shuffle=False))
        assert len(got) == 2 and torch.equal(got[0][0], images[:2]) and torch.equal(got[1][1], masks[2:4].long())
        assert list(ds.batches(2, shuffle=False, augment=None))[0][2].tolist() == [0, 1]

        pet = DevicePetDataset.__new__(DevicePetDataset)          # the tensors of a decoded dataset, without the decode
        pet.device = torch.device("cpu")
        pet.images = torch.randint(0, 256, (5, 3, 8, 8), generator=g).to(torch.uint8)
        pet.trimaps = torch.randint(1, 4, (5, 8, 8), generator=g).to(torch.uint8)
        pet.categories = torch.zeros(5, dtype=torch.int64)
        pet._table = _to_float_table()
        loader = DeviceLoader(pet, 2)
        assert loader.augment is None
        batches = list(loader)
        assert len(batches) == 3 and torch.equal(batches[0][1], (pet.trimaps[:2] == 1).long())
        assert torch.equal(batches[0][0], pet.images[:2].float().div(255))
        assert "weaklysuperviseddl_amd.augment" not in sys.modules
    finally:
        sys.modules["weaklysuperviseddl_amd.augment"] = saved


def test_train_step_signature_has_the_ignore_label():
    import inspect
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import train_step
    p = inspect.signature(train_step).parameters["ignore_label"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
