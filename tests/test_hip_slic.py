"""Integer SLIC superpixels, their connectivity pass and the pooling over them (csrc/slic.hip) against the numpy + scipy oracle of
tests/slic_oracle.py.  Everything is EQUAL, never close: the label maps, the centres, the segment ids and their number, and the
pooled floats bit for bit (NaNs at the same places)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def T(a):
    """A torch copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def case_name(c):
    content, shape, m, it, ms = c
    return f"{content}-{'x'.join(str(v) for v in shape)}-m{m}-it{it}-min{ms}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_slic(dev, images, step, **kw):
    from weaklysuperviseddl_amd import ops
    out = {}
    seg, n = ops.slic(T(images).to(dev), step, out=out, **kw)
    assert int(out["error"].item()) == 0
    return {k: out[k].cpu().numpy() for k in ("raw", "centres", "segments", "n_segments")}


# ------------------------------------------------------------------------------------------------ 1. slic
@pytest.mark.parametrize("c", so.device_cases(), ids=case_name)
def test_slic_equals_the_oracle(dev, c):
    from weaklysuperviseddl_amd import ops
    content, shape, m, it, ms = c
    B, H, W, step = shape
    images, want, stats = so.case(*c)
    img = T(images).to(dev)
    before = img.clone()
    out = {}
    seg, n = ops.slic(img, step, m, it, ms, out=out)
    assert seg.dtype == torch.int32 and n.dtype == torch.int32 and out["segments"] is seg and out["n_segments"] is n
    assert out["raw"].dtype == torch.int32 and out["centres"].dtype == torch.int32
    assert int(out["error"].item()) == 0
    got = {k: out[k].cpu().numpy() for k in want}
    for k in ("raw", "centres", "n_segments", "segments"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, case_name(c), int((got[k] != want[k]).sum()))
    assert got["n_segments"].max() <= ops.slic_max_segments(H, W, step, ms)
    assert torch.equal(img, before)                                         # the images are never written
    # the out= buffers are reused at the same addresses and a second call is bit-identical
    ptrs = {k: out[k].data_ptr() for k in want}
    seg2, n2 = ops.slic(img, step, m, it, ms, out=out)
    assert {k: out[k].data_ptr() for k in want} == ptrs and seg2 is seg and n2 is n
    for k in want:
        assert np.array_equal(out[k].cpu().numpy(), got[k]), k


def test_identical_images_give_identical_maps_and_different_ones_do_not(dev):
    same = device_slic(dev, so.structured_images()["same3"], 10)
    for k in ("raw", "centres", "segments"):
        assert np.array_equal(same[k][0], same[k][1]) and np.array_equal(same[k][0], same[k][2]), k
    diff = device_slic(dev, so.structured_images()["different3"], 10)
    assert not np.array_equal(diff["segments"][0], diff["segments"][1])
    assert np.array_equal(diff["segments"][0], same["segments"][0])        # image 0 is the same blob image: no cross-talk in a batch


def test_quantize_then_slic(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 3, 37, 53, generator=g) * 1.3).to(dev)
    x[0, :, :10] = 9.0                                                      # clamps to 255
    x[1, :, 20:] = -9.0                                                     # clamps to 0
    q = ops.slic_quantize(x)
    mean = torch.tensor(ops._SLIC_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(ops._SLIC_STD, device=dev).view(1, 3, 1, 1)
    same = torch.clamp(torch.round((x * std + mean) * 255), 0, 255).to(torch.uint8)
    assert q.dtype == torch.uint8 and torch.equal(q, same) and q.min() == 0 and q.max() == 255
    want = so.slic(same.cpu().numpy(), 8)
    from weaklysuperviseddl_amd import nn as wnn
    seg, n = wnn.Superpixels(8)(x)
    assert np.array_equal(seg.cpu().numpy(), want["segments"]) and np.array_equal(n.cpu().numpy(), want["n_segments"])
    seg_u8, _ = wnn.Superpixels(8)(q)
    assert torch.equal(seg, seg_u8) and seg.grad_fn is None


def test_refusals(dev):
    from weaklysuperviseddl_amd import ops, _lib
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev)
    for step in (0, 129):
        with pytest.raises(ValueError):
            ops.slic(img, step)
    with pytest.raises(ValueError):
        ops.slic(img.float(), 4)
    with pytest.raises(ops.WsdlError):
        ops.slic(img.cpu(), 4)                                              # a host tensor: there is no CPU fallback
    lib = _lib.lib()
    need = lib.wsdl_slic_workspace(1, 8, 8, 4)
    assert need > 0 and lib.wsdl_slic_workspace(1, 8, 8, 0) == 0 and lib.wsdl_slic_workspace(1, 8, 8, 129) == 0
    assert lib.wsdl_slic_workspace(1, 8193, 8, 4) == 0
    raw = torch.empty(1, 8, 8, dtype=torch.int32, device=dev)
    seg = torch.empty_like(raw)
    cen = torch.empty(1, 4, 5, dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = lambda step, m, it, ms, nbytes: (img.data_ptr(), 1, 8, 8, step, m, it, ms, raw.data_ptr(), cen.data_ptr(),    # noqa: E731
                                            seg.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes, None)
    assert lib.wsdl_slic(*args(4, 10, 2, 4, need - 1)) != 0 and b"workspace" in lib.wsdl_last_error()
    assert lib.wsdl_slic(*args(0, 10, 2, 4, need)) != 0 and lib.wsdl_slic(*args(129, 10, 2, 4, need)) != 0
    assert lib.wsdl_slic(*args(4, 0, 2, 4, need)) != 0 and b"compactness" in lib.wsdl_last_error()
    assert lib.wsdl_slic(*args(4, 10, -1, 4, need)) != 0 and lib.wsdl_slic(*args(4, 10, 2, 0, need)) != 0
    assert lib.wsdl_slic(*args(4, 10, 2, 4, need)) == 0                     # and the same call with enough scratch runs
    assert np.array_equal(seg.cpu().numpy(), so.slic(np.zeros((1, 3, 8, 8), dtype=np.uint8), 4, 10, 2, 4)["segments"])


# ------------------------------------------------------------------------------------------------ 2. pooling
def pooling_inputs(C, seed):
    """Segments of a noise image (many small ones), values with the awkward entries of the contract."""
    _, want, _ = so.case("different3", (2, 65, 130, 10))
    seg = np.array(want["segments"])
    B, H, W = seg.shape
    n_max = so.max_segments(H, W, 10) + 3                                   # ids past every n_b: empty segments
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((B, C, H, W)).astype(np.float32)
    v[0, 0, 3, 5] = np.nan                                                  # a NaN pixel: its (image, channel, segment) only
    v[1, C - 1, 40, 100] = np.nan
    v[0, 0, 10, 10:14] = [40000.0, -40000.0, 32768.0, -32768.0]             # beyond +-2^15: clamped
    v[2, 0, 20, 20:23] = [np.inf, -np.inf, 1e-9]
    v[1, 0, 30, :] = np.float32(2.0 ** -25) * 3                             # below half a quantum and ties of the rounding
    v[2, C - 1, 50:60] *= 1000.0
    return v, seg, n_max


@pytest.mark.parametrize("C", (1, 2, 21))
def test_superpixel_mean_and_snap_equal_the_oracle_bit_for_bit(dev, C):
    from weaklysuperviseddl_amd import ops
    v, seg, n_max = pooling_inputs(C, C)
    want_mean, want_count = so.superpixel_mean(v, seg, n_max)
    assert (want_count == 0).any() and np.isnan(want_mean).sum() == 2 and want_count.sum() == seg.size
    vd, sd = T(v).to(dev), T(seg).to(dev)
    v0, s0 = vd.clone(), sd.clone()
    out = {}
    mean, count = ops.superpixel_mean(vd, sd, n_max, out=out)
    assert mean.dtype == torch.float32 and count.dtype == torch.int32 and tuple(mean.shape) == (seg.shape[0], C, n_max)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(bits(mean.cpu().numpy()), bits(want_mean)), int((bits(mean.cpu().numpy()) != bits(want_mean)).sum())
    snapped = ops.superpixel_snap(vd, sd, n_max, out=out)
    assert out["mean"] is mean and out["count"] is count and snapped.shape == vd.shape
    assert np.array_equal(bits(snapped.cpu().numpy()), bits(so.superpixel_snap(v, seg, n_max)))
    assert np.array_equal(bits(out["mean"].cpu().numpy()), bits(want_mean))   # a second pass over the same buffers: the same bits
    vb, sb = vd.view(torch.int32), sd
    assert torch.equal(vb, v0.view(torch.int32)) and torch.equal(sb, s0)    # the inputs are never written
    # ids outside [0, n_max) are not pooled and snap to 0
    small = 50
    m2, c2 = ops.superpixel_mean(vd, sd, small)
    wm2, wc2 = so.superpixel_mean(v, seg, small)
    assert np.array_equal(c2.cpu().numpy(), wc2) and np.array_equal(bits(m2.cpu().numpy()), bits(wm2))
    assert np.array_equal(bits(ops.superpixel_snap(vd, sd, small).cpu().numpy()), bits(so.superpixel_snap(v, seg, small)))


def test_superpixel_vote_equals_the_oracle(dev):
    from weaklysuperviseddl_amd import ops
    _, want, _ = so.case("different3", (2, 65, 130, 10))
    seg = np.array(want["segments"])
    B, H, W = seg.shape
    n_max = so.max_segments(H, W, 10)
    rng = np.random.default_rng(9)
    for NC in (2, 3, 64):
        lab = rng.integers(0, NC, seg.shape).astype(np.int64)
        lab[rng.random(seg.shape) < 0.2] = 255                              # ignored pixels
        lab[0][seg[0] == 3] = 255                                           # an all-ignore segment
        lab[0][seg[0] == 4] = -1
        ids = np.flatnonzero(seg[1] == 5)                                   # a tie between the two largest classes
        lab[1].ravel()[ids] = 255
        lab[1].ravel()[ids[:2]] = [NC - 1, 0]
        wantv = so.superpixel_vote(lab, seg, n_max, NC)
        assert (wantv[0][seg[0] == 3] == 255).all() and (wantv[1][seg[1] == 5] == 0).all() and len(ids) >= 2
        ld, sd = T(lab).to(dev), T(seg).to(dev)
        got = ops.superpixel_vote(ld, sd, n_max, NC)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), wantv), NC
        assert np.array_equal(ops.superpixel_vote(ld, sd, n_max, NC, ignore_index=-100).cpu().numpy(),
                              so.superpixel_vote(lab, seg, n_max, NC, ignore_index=-100))
        assert np.array_equal(ld.cpu().numpy(), lab)
    from weaklysuperviseddl_amd import nn as wnn
    images = so.structured_images()["different3"]
    lab = rng.integers(0, 2, seg.shape).astype(np.int64)
    got = wnn.Superpixels(10).vote(T(images).to(dev), T(lab).to(dev), 2)
    assert np.array_equal(got.cpu().numpy(), so.superpixel_vote(lab, seg, n_max, 2))
    sc = rng.standard_normal((B, 2, H, W)).astype(np.float32)
    got = wnn.Superpixels(10).snap(T(images).to(dev), T(sc).to(dev))
    assert np.array_equal(bits(got.cpu().numpy()), bits(so.superpixel_snap(sc, seg, n_max)))


# ------------------------------------------------------------------------------------------------ 3. launch plan
def test_a_plan_replays_slic_on_new_contents(dev):
    from weaklysuperviseddl_amd import ops, plan
    shape, it = (2, 65, 130, 10), 3
    a, want_a, _ = so.case("blobs", shape, 10, it)
    b, want_b, _ = so.case("noise", shape, 10, it)
    img = T(a).to(dev)
    out = {}
    ops.slic(img, 10, num_iter=it, out=out)                                 # the scratch buffer exists before the recording
    p, _ = plan.record(ops.slic, img, 10, num_iter=it, out=out)
    assert p.stats["kernels"] == ops.slic_launches(65, 130, it) == 8 + 4 + 2 * it and p.stats["memsets"] == 0
    for k in want_a:
        assert np.array_equal(out[k].cpu().numpy(), want_a[k]), k
    img.copy_(T(b).to(dev))
    for k in ("segments", "raw", "centres", "n_segments"):
        out[k].fill_(-5)
    p.replay()
    for k in want_b:
        assert np.array_equal(out[k].cpu().numpy(), want_b[k]), k
    assert int(out["error"].item()) == 0
    # one labelling tile: a launch fewer; no iteration: one assignment
    small = torch.zeros(1, 3, 20, 30, dtype=torch.uint8, device=dev)
    p2, _ = plan.record(ops.slic, small, 64, num_iter=0)
    assert p2.stats["kernels"] == ops.slic_launches(20, 30, 0) == 8 + 3 + 1


# ------------------------------------------------------------------------------------------------ 4. where it surfaces
class _FakeCam:
    """What ``generate_pseudo_masks`` needs of a LayerCAM generator: a smooth CAM from the images and its thresholded mask."""

    def generate_batch(self, imgs, alpha=1.0, class_idx=None, thresh=None):
        cam = torch.sigmoid(imgs.mean(dim=1) * 2.0).contiguous()
        return cam, (cam >= thresh).to(torch.uint8)


def _loader(n_batches, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_batches):
        x = torch.randn(B, 3, H, W, generator=g)
        x = torch.nn.functional.avg_pool2d(x, 9, 1, 4) * 6
        out.append((x, (torch.zeros(B, dtype=torch.int64), None)))
    return out


def test_generate_pseudo_masks_with_superpixels(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import PsuedoMasks as pm
    loader = _loader(2, 3, 48, 80, 1)
    gen = _FakeCam()
    kw = dict(cam_thresh=0.5, write_png=False, device=dev, keep_on_device=True)
    pm.generate_pseudo_masks(loader, gen, **kw)
    base = [m.clone() for m in pm.generate_pseudo_masks.last_masks]
    pm.generate_pseudo_masks(loader, gen, superpixels=None, **kw)
    again = pm.generate_pseudo_masks.last_masks
    want = torch.cat([ops.keep_largest_batched(gen.generate_batch(x.to(dev), thresh=0.5)[1]) for x, _ in loader])
    assert len(base) == 6 and all(torch.equal(a, b) for a, b in zip(base, again)) and torch.equal(torch.stack(base), want)
    sp = {"step": 8, "compactness": 20}
    pm.generate_pseudo_masks(loader, gen, superpixels=sp, **kw)
    got = torch.stack(pm.generate_pseudo_masks.last_masks)
    comp = []
    for x, _ in loader:
        xd = x.to(dev)
        cam, _ = gen.generate_batch(xd, thresh=0.5)
        seg, _ = ops.slic(ops.slic_quantize(xd), **sp)
        snapped = ops.superpixel_snap(cam[:, None], seg, ops.slic_max_segments(48, 80, 8))[:, 0]
        comp.append(ops.keep_largest_batched((snapped >= 0.5).to(torch.uint8)))
    assert torch.equal(got, torch.cat(comp)) and not torch.equal(got, want) and got.sum() > 0
    with pytest.raises(ValueError):
        pm.generate_pseudo_masks(loader, gen, superpixels=sp, pamr={}, **kw)
    with pytest.raises(ValueError):
        pm.generate_pseudo_masks(loader, gen, superpixels={"step": 0}, **kw)


def test_refine_dataset_with_superpixels(dev):
    from conftest import smooth_image
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import InMemoryPseudoDataset, build_segmentation_model, refine_dataset
    from weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss import network_soft_prediction
    torch.manual_seed(0)
    model = build_segmentation_model()
    for mod in model.modules():
        if isinstance(mod, wnn.Dropout):
            mod.p = 0.0
    model = model.to(dev).train()
    img = smooth_image(4, 32, 32, 7)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    masks = (img[:, 0] > 0.5).to(torch.uint8) * 255
    images = ((img - mean) / std).to(dev)

    def data():
        return InMemoryPseudoDataset(images.clone(), masks.to(dev))

    S = network_soft_prediction(model, images)
    thr = S[:, 1].median().item()                                           # (a threshold that splits the toy prediction)
    # the default method is the call without the new arguments, bit for bit
    a = refine_dataset(model, data(), repeats=1, chunk=4, threshold=thr, num_steps=2).masks
    b = refine_dataset(model, data(), repeats=1, chunk=4, threshold=thr, num_steps=2, method="ncut", superpixel_kwargs=None).masks
    assert torch.equal(a, b)
    sp = {"step": 8, "num_iter": 4, "compactness": 5}
    ds = refine_dataset(model, data(), repeats=3, chunk=4, threshold=thr, method="superpixel", superpixel_kwargs=sp)
    seg, n = ops.slic(ops.slic_quantize(images), **sp)
    want = (ops.superpixel_snap(S, seg, ops.slic_max_segments(32, 32, 8))[:, 1] > thr).to(torch.uint8) * 255
    assert torch.equal(ds.masks, want) and 0 < int((want > 0).sum()) < want.numel() and int(n.min()) > 1
    with pytest.raises(ValueError):
        refine_dataset(model, data(), method="slic")
