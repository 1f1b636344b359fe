"""Dense-CRF refinement (reference AlternatingDirectionCutLoss.py:183-204): the CPU oracle's semantics (tests/crf_oracle.py)
and the device path (csrc/crf.hip, ops.dense_crf, the drop-in apply_dense_crf / generate_crf_pseudo_masks) against it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crf_oracle as co  # noqa: E402
from conftest import report_line, smooth_image  # noqa: E402


def _rgb(B, H, W, seed, noise=False):
    """(B,H,W,3) uint8 the notebook's way: truncation of x*255."""
    if noise:
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))
    else:
        x = smooth_image(B, H, W, seed)
    return np.stack([co.quantise(x[b].numpy()) for b in range(B)])


def _cam(B, H, W, seed):
    """Smooth CAM-like maps in [0,1] with a blob of foreground."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for _ in range(B):
        cy, cx, r = g.uniform(0.3, 0.7) * H, g.uniform(0.3, 0.7) * W, g.uniform(0.2, 0.4) * max(H, W)
        c = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)) + 0.15 * g.rand(H, W)
        out.append((c / c.max()).astype(np.float32))
    return np.stack(out)


# ---- CPU: the oracle's semantics ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bilateral", [False, True])
def test_oracle_vertices_and_weights(bilateral):
    rgb = _rgb(1, 32, 40, 1)[0]
    f = co.crf_features(rgb, 50, 5) if bilateral else co.crf_features(rgb, 1)
    keys, bary = co.lattice_coords(f)
    D = f.shape[1] + 1
    # d+1 distinct vertices per pixel
    for r in range(D):
        for s in range(r + 1, D):
            assert (keys[:, r] != keys[:, s]).any(1).all()
    assert bary.min() >= -2e-7
    assert np.abs(bary.astype(np.float64).sum(1) - 1).max() < 4e-7
    # each vertex lies on the lattice: the d+1 coordinates (the last is minus the sum) are congruent mod d+1
    full = np.concatenate([keys, -keys.sum(2, keepdims=True)], 2)
    assert ((full - full[:, :, :1]) % D == 0).all()


@pytest.mark.parametrize("bilateral", [False, True])
def test_oracle_filter_symmetric(bilateral):
    """Each axis' blur is symmetric (n2 of n1 is the point itself) and the filter with the blur axes reversed is exactly the
    transpose of the forward one.  The forward filter alone is not symmetric on a sparse lattice: the per-axis blurs do not
    commute where neighbours are missing (densecrf filters the transpose with its `reverse` flag for that reason) - on the
    12 x 12 image below its largest asymmetry is 0.19 (Gaussian) / 0.14 (bilateral) of the largest entry."""
    rgb = _rgb(1, 12, 12, 2, noise=True)[0]
    f = co.crf_features(rgb, 3, 20) if bilateral else co.crf_features(rgb, 1.5)
    lat = co.Lattice(f)
    for n1, n2 in lat.nbr:
        has = n1 < lat.M
        assert np.array_equal(n2[n1[has]], np.arange(lat.M)[has])
    eye = np.eye(len(f))
    K, Kr = lat.apply(eye), lat.apply(eye, reverse=True)
    assert np.abs(Kr - K.T).max() < 1e-12 * np.abs(K).max()
    # the symmetric normalisation keeps that relation: K~ with reversed blurs = K~^T
    n = 1.0 / np.sqrt(lat.apply(np.ones((len(f), 1)))[:, 0] + 1e-20)
    Kn, Knr = n[:, None] * K * n[None, :], n[:, None] * Kr * n[None, :]
    assert np.abs(Knr - Kn.T).max() < 1e-12 * np.abs(Kn).max()
    asym = np.abs(K - K.T).max() / np.abs(K).max()
    report_line(f"dense CRF lattice filter asymmetry on 12x12 ({'bilateral' if bilateral else 'gaussian'}): {asym:.3f}")
    assert asym < 0.3


# relative L2 gap of the normalised lattice filter to the exact dense Gaussian on a 24 x 24 smooth image, measured:
# Gaussian (sxy 1) 0.0197, bilateral (sxy 50, srgb 5) 0.0769.  A wrong lattice scale moves them far (features x 1.5: 0.113 /
# 0.159 - test_oracle_wrong_scale_is_visible); alpha cancels in the symmetric normalisation.
GAP = {False: 0.0197, True: 0.0769}


def _gap(bilateral, scale=None):
    rgb = _rgb(1, 24, 24, 3)[0]
    f = co.crf_features(rgb, 50, 5) if bilateral else co.crf_features(rgb, 1)
    x = np.random.RandomState(0).rand(len(f), 2)
    exact = co.NormalisedFilter(f, exact=True)(x)
    lat = co.NormalisedFilter(f if scale is None else f * np.float32(scale))(x)
    return np.linalg.norm(lat - exact) / np.linalg.norm(exact)


@pytest.mark.parametrize("bilateral", [False, True])
def test_oracle_filter_tracks_exact_gaussian(bilateral):
    gap = _gap(bilateral)
    report_line(f"dense CRF lattice vs exact Gaussian, 24x24, {'bilateral' if bilateral else 'gaussian'}: rel L2 {gap:.4f}")
    assert gap < 1.3 * GAP[bilateral], gap


def test_oracle_wrong_scale_is_visible():
    for bilateral in (False, True):
        assert _gap(bilateral, 1.5) > 1.8 * GAP[bilateral]


def test_oracle_zero_compat_is_argmax_of_probs():
    rgb = _rgb(1, 20, 28, 4)[0]
    cam = _cam(1, 20, 28, 4)[0]
    mask, _ = co.dense_crf(rgb, cam, 0.2, gauss=(1, 0), bilateral=(50, 5, 0))
    c = cam.copy()
    c[c < np.float32(0.2)] = 0
    probs = np.clip(np.stack([1 - c, c]), 1e-8, 1)
    assert np.array_equal(mask, np.argmax(probs, 0).astype(np.uint8))


def test_oracle_masks_vs_exact_filter_mean_field():
    agree = []
    for seed in range(3):
        rgb = _rgb(1, 24, 24, 10 + seed)[0]
        cam = _cam(1, 24, 24, 10 + seed)[0]
        m_lat, _ = co.dense_crf(rgb, cam, 0.2)
        m_ex, _ = co.dense_crf(rgb, cam, 0.2, exact=True)
        agree.append((m_lat == m_ex).mean())
    report_line("dense CRF masks, lattice vs exact-filter mean field, 24x24 x 3: agreement %s" % ", ".join("%.4f" % a for a in agree))
    assert min(agree) >= 0.98, agree


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _oracle_batch(rgb, cam, cam_thresh=0.2, **kw):
    ms, qs = zip(*[co.dense_crf(rgb[b], cam[b], cam_thresh, **kw) for b in range(len(rgb))])
    return np.stack(ms), np.stack(qs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["smooth224", "noise224", "odd37x53"])
def test_lattice_equals_oracle(dev, case):
    from weaklysuperviseddl_amd import ops
    B, H, W = (3, 224, 224) if case != "odd37x53" else (2, 37, 53)
    rgb = _rgb(B, H, W, 7, noise=case == "noise224")
    for bilateral, sxy, srgb in ((False, 1.0, 1.0), (True, 50.0, 5.0)):
        keys, bary, points = ops.dense_crf_lattice(torch.from_numpy(rgb).to(dev), bilateral, sxy, srgb)
        keys, bary, points = keys.cpu().numpy(), bary.cpu().numpy(), points.cpu().numpy()
        N = H * W
        for b in range(B):
            f = co.crf_features(rgb[b], sxy, srgb) if bilateral else co.crf_features(rgb[b], sxy)
            lat = co.Lattice(f)
            assert np.array_equal(keys[b * N:(b + 1) * N], lat.keys), (case, bilateral, b)
            assert np.array_equal(bary[b * N:(b + 1) * N].view(np.uint32), lat.bary.view(np.uint32)), (case, bilateral, b)
            assert points[b] == lat.M, (case, bilateral, b, points[b], lat.M)


@pytest.mark.gpu
@pytest.mark.parametrize("bilateral", [False, True])
def test_one_filter_application(dev, bilateral):
    from weaklysuperviseddl_amd import ops
    B, H, W = 2, 64, 72
    rgb = _rgb(B, H, W, 8)
    x = np.random.RandomState(1).rand(B, 2, H, W).astype(np.float32)
    sxy, srgb = (50.0, 5.0) if bilateral else (1.0, 1.0)
    out = ops.dense_crf_filter(torch.from_numpy(rgb).to(dev), torch.from_numpy(x).to(dev), bilateral, sxy, srgb).cpu().numpy()
    for b in range(B):
        f = co.crf_features(rgb[b], sxy, srgb) if bilateral else co.crf_features(rgb[b], sxy)
        ref = co.NormalisedFilter(f)(x[b].reshape(2, -1).T).T.reshape(2, H, W)
        err = np.abs(out[b] - ref).max() / np.abs(ref).max()
        assert err < 1e-5, (bilateral, b, err)


def _check_inference(dev, rgb, cam, label, cam_thresh=0.2):
    from weaklysuperviseddl_amd import ops
    mask, q = ops.dense_crf(torch.from_numpy(rgb).to(dev), torch.from_numpy(cam).to(dev), cam_thresh=cam_thresh, return_q=True)
    mask, q = mask.cpu().numpy(), q.cpu().numpy()
    m_ref, q_ref = _oracle_batch(rgb, cam, cam_thresh)
    assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    dq = np.abs(q - q_ref).max()
    assert dq < 1e-4, (label, dq)
    close = np.abs(q_ref[:, 1] - q_ref[:, 0]) < 1e-4
    diff = mask != m_ref
    assert not (diff & ~close).any(), (label, int((diff & ~close).sum()))
    report_line(f"dense CRF {label}: max |dQ| {dq:.2e}, mask pixels differing {int(diff.sum())} of {mask.size} "
                f"({int(close.sum())} oracle pixels with |Q1-Q0| < 1e-4)")
    return mask, q


@pytest.mark.gpu
def test_inference_matches_oracle(dev):
    B, H, W = 3, 224, 224
    _check_inference(dev, _rgb(B, H, W, 11), _cam(B, H, W, 11), "224x224 B=3")
    _check_inference(dev, _rgb(2, 37, 53, 12, noise=True), _cam(2, 37, 53, 12), "37x53 noise B=2")


@pytest.mark.gpu
def test_inference_edge_inputs(dev):
    H, W = 40, 48
    rgb = _rgb(2, H, W, 13)
    zero, one = np.zeros((2, H, W), np.float32), np.ones((2, H, W), np.float32)
    m0, _ = _check_inference(dev, rgb, zero, "all-zero CAM")
    assert (m0 == 0).all()
    m1, _ = _check_inference(dev, rgb, one, "all-one CAM")
    assert (m1 == 1).all()
    flat = np.full((2, H, W, 3), 97, np.uint8)
    _check_inference(dev, flat, _cam(2, H, W, 14), "constant image")
    _check_inference(dev, _rgb(2, 1, 57, 15), _cam(2, 1, 57, 15), "H=1")


@pytest.mark.gpu
def test_deterministic_and_batch_independent(dev):
    from weaklysuperviseddl_amd import ops
    B, H, W = 8, 96, 112
    rgb = torch.from_numpy(_rgb(B, H, W, 16)).to(dev)
    cam = torch.from_numpy(_cam(B, H, W, 16)).to(dev)
    m1, q1 = ops.dense_crf(rgb, cam, cam_thresh=0.2, return_q=True)
    m2, q2 = ops.dense_crf(rgb, cam, cam_thresh=0.2, return_q=True)
    assert torch.equal(m1, m2) and torch.equal(q1.view(torch.int32), q2.view(torch.int32))
    for b in range(B):
        mb, qb = ops.dense_crf(rgb[b:b + 1], cam[b:b + 1], cam_thresh=0.2, return_q=True)
        assert torch.equal(mb[0], m1[b]) and torch.equal(qb[0].view(torch.int32), q1[b].view(torch.int32)), b


@pytest.mark.gpu
def test_float_images_are_quantised_by_truncation(dev):
    from weaklysuperviseddl_amd import ops
    x = smooth_image(2, 30, 34, 17)
    rgb = np.stack([co.quantise(x[b].numpy()) for b in range(2)])
    cam = torch.from_numpy(_cam(2, 30, 34, 17)).to(dev)
    m_f, q_f = ops.dense_crf(x.to(dev), cam, cam_thresh=0.2, return_q=True)
    m_u, q_u = ops.dense_crf(torch.from_numpy(rgb).to(dev), cam, cam_thresh=0.2, return_q=True)
    assert torch.equal(m_f, m_u) and torch.equal(q_f, q_u)


@pytest.mark.gpu
def test_apply_dense_crf_drop_in(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import apply_dense_crf
    H, W = 50, 64
    rgb = _rgb(1, H, W, 18)[0]
    cam = _cam(1, H, W, 18)[0]
    cam[cam < 0.2] = 0
    out = apply_dense_crf(rgb, cam)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (H, W) and set(np.unique(out)) <= {0, 1}
    ref = ops.dense_crf(torch.from_numpy(rgb).to(dev)[None], torch.from_numpy(cam).to(dev)[None])[0].cpu().numpy()
    assert np.array_equal(out, ref)
    # a non-contiguous image (a channel-last view of a CHW array, as permute(1, 2, 0).numpy() gives)
    chw = np.ascontiguousarray(rgb.transpose(2, 0, 1))
    view = chw.transpose(1, 2, 0)
    assert not view.flags["C_CONTIGUOUS"]
    assert np.array_equal(apply_dense_crf(view, cam), out)


class _TinyLoader:
    def __init__(self, imgs, labels, bs):
        self.imgs, self.labels, self.bs = imgs, labels, bs

    def __iter__(self):
        for s in range(0, len(self.imgs), self.bs):
            yield self.imgs[s:s + self.bs], (self.labels[s:s + self.bs], None)


@pytest.mark.gpu
def test_generate_crf_pseudo_masks(dev, tmp_path):
    from PIL import Image
    from weaklysuperviseddl_amd.TraditionalModel import (FrozenResNetCAM, LayerCAMGenerator, PseudoSegmentationDataset,
                                                         generate_crf_pseudo_masks)
    torch.manual_seed(0)
    model = FrozenResNetCAM(num_classes=5).to(dev).eval()
    H = W = 64
    gen = LayerCAMGenerator(model, ["layer3", "layer4"], variant="notebook", out_hw=(H, W))
    imgs = smooth_image(5, H, W, 19)
    labels = torch.tensor([0, 3, 1, 4, 2])
    loader = _TinyLoader(imgs, labels, 2)
    idir, mdir = generate_crf_pseudo_masks(loader, gen, alpha=0.5, cam_thresh=0.2, out_root=str(tmp_path), max_images=4,
                                           device=dev)
    assert sorted(os.listdir(mdir)) == ["0.png", "1.png", "2.png", "3.png"] == sorted(os.listdir(idir))
    cams = [c.cpu().numpy() for c in generate_crf_pseudo_masks.last_cams]
    assert len(cams) == 4
    n_fg = 0
    for i in range(4):
        rgb = co.quantise(imgs[i].numpy())
        m_ref, q_ref = co.dense_crf(rgb, cams[i], 0.2)
        png = np.asarray(Image.open(os.path.join(mdir, f"{i}.png")).convert("L"))
        close = np.abs(q_ref[1] - q_ref[0]) < 1e-4
        diff = (png != m_ref.astype(np.uint8) * 255)
        assert set(np.unique(png)) <= {0, 255}
        assert not (diff & ~close).any(), i
        n_fg += int((png == 255).sum())
    report_line(f"generate_crf_pseudo_masks: 4 masks of 64x64 equal to the oracle CRF ({n_fg} foreground pixels)")
    ds = PseudoSegmentationDataset(idir, mdir, transform=True)
    assert len(ds) == 4
    img_t, mask_t = ds[0]
    assert tuple(img_t.shape) == (3, 256, 256) and tuple(mask_t.shape) == (256, 256)
    assert set(torch.unique(mask_t).tolist()) <= {0, 255}


@pytest.mark.gpu
def test_refusals(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd._lib import WsdlError, lib
    rgb = torch.from_numpy(_rgb(1, 16, 16, 20)).to(dev)
    cam = torch.from_numpy(_cam(1, 16, 16, 20)).to(dev)
    with pytest.raises(WsdlError):
        ops.dense_crf(rgb.cpu(), cam.cpu())                      # off the device
    with pytest.raises(WsdlError):
        ops.dense_crf(rgb, cam.double())                         # wrong dtype
    with pytest.raises(WsdlError):
        ops.dense_crf(rgb.to(torch.int32), cam)
    with pytest.raises(WsdlError):
        ops.dense_crf(rgb, unary=torch.zeros(1, 3, 16, 16, device=dev), n_labels=3)
    # the C ABI refuses n_labels != 2 before launching anything
    ws = torch.empty(lib().wsdl_dense_crf_workspace(1, 16, 16, 2), dtype=torch.uint8, device=dev)
    mask = torch.empty(1, 16, 16, dtype=torch.uint8, device=dev)
    rc = lib().wsdl_dense_crf(rgb.data_ptr(), cam.data_ptr(), None, 0.2, 1, 16, 16, 3, 5, 1.0, 2.0, 50.0, 5.0, 10.0,
                              mask.data_ptr(), None, ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b"n_labels" in lib().wsdl_last_error()
    assert lib().wsdl_dense_crf_workspace(1, 16, 16, 3) == 0
