"""BASNet saliency inference (reference PretrainedBasnetModel/): the model's parameter names, the float64 oracle against the
reference bodies' fixture (tests/golden/basnet.npz), the device forward and its kernels (csrc/basnet.hip) against both, and the
Pet evaluation drop-in (RunInference.run_inference)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import basnet_oracle as bo  # noqa: E402
from conftest import GOLDEN, ROOT, report_line  # noqa: E402


def _fixture():
    z = np.load(os.path.join(GOLDEN, "basnet.npz"))
    keys = [str(k) for k in z["keys"]]
    shapes = [tuple(int(d) for d in row[1:1 + row[0]]) for row in z["shapes"]]
    stats = {k[len("stat/"):]: z[k] for k in z.files if k.startswith("stat/")}
    cases = [(z[f"case{i}/input_u8"], z[f"case{i}/outputs"]) for i in range(len(bo.CASES))]
    return list(zip(keys, shapes)), stats, cases


def _state_dict():
    ks, stats, _ = _fixture()
    return bo.seeded_state_dict(ks, stats)


# ----------------------------------------------------------------------------------------------------------- CPU
def test_state_dict_names_and_shapes_match_reference():
    from weaklysuperviseddl_amd.PretrainedBasnetModel.model import BASNet
    ks, _, _ = _fixture()
    net = BASNet(3, 1)
    mine = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert sorted(mine) == sorted(ks)
    net.load_state_dict(_state_dict(), strict=True)
    # biases exactly where the reference has them
    sd = net.state_dict()
    assert "inconv.bias" in sd and "conv6d_1.bias" in sd and "refunet.conv0.bias" in sd and "outconvb.bias" in sd
    assert "encoder1.0.conv1.bias" not in sd and "encoder2.0.downsample.0.bias" not in sd


def test_import_and_construct_without_torchvision():
    code = ("import sys; sys.path.insert(0, %r); from weaklysuperviseddl_amd.PretrainedBasnetModel.model import BASNet; "
            "BASNet(3, 1); import weaklysuperviseddl_amd.PretrainedBasnetModel.RunInference; "
            "assert 'torchvision' not in sys.modules, 'torchvision imported'" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_oracle_matches_reference_fixture():
    _, _, cases = _fixture()
    sd = _state_dict()
    worst = 0.0
    for u8, ref in cases:
        with torch.no_grad():
            ys = bo.forward(sd, bo.input_batch(u8))
        got = torch.stack(ys).numpy()
        assert got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
    assert worst <= 1e-6, worst


def test_compute_metrics_and_norm_pred():
    from weaklysuperviseddl_amd.PretrainedBasnetModel import RunInference as ri
    pred = np.array([[0.2, 0.7], [0.9, 0.1]])
    gt = np.array([[1, 1], [2, 3]])
    iou, acc, pb, gb = ri.compute_metrics(pred, gt)
    assert iou == pytest.approx(1 / 3) and acc == pytest.approx(0.5)
    assert pb.dtype == np.uint8 and gb.tolist() == [[1, 1], [0, 0]]
    iou, acc, _, _ = ri.compute_metrics(np.zeros((3, 3)), np.full((3, 3), 2))      # empty union
    assert iou == 1.0 and acc == 1.0
    d = torch.full((1, 4, 4), 0.3)                                                    # all equal: 0 / 1e-8
    assert torch.equal(ri.norm_pred(d), torch.zeros_like(d))
    d = torch.tensor([[1.0, 3.0], [2.0, 5.0]])
    assert torch.allclose(ri.norm_pred(d), (d - 1) / (4 + 1e-8))


# ----------------------------------------------------------------------------------------------------------- GPU
def _dev_net(sd=None):
    from weaklysuperviseddl_amd.PretrainedBasnetModel.model import BASNet
    net = BASNet(3, 1)
    net.load_state_dict(sd if sd is not None else _state_dict())
    return net.cuda().eval()


@pytest.mark.gpu
def test_network_matches_reference_fixture():
    _, _, cases = _fixture()
    net = _dev_net()
    worst = []
    for u8, ref in cases:
        with torch.no_grad():
            ys = net(bo.input_batch(u8).cuda())
        got = torch.stack(ys).cpu().numpy()
        errs = np.abs(got - ref).reshape(8, -1).max(1)
        worst.append(errs)
        assert errs.max() <= 1e-4, errs
    report_line("BASNet vs the reference bodies' fixture (64x64 B=2, 96x128 B=1): worst |sigmoid| error per output "
                "(dout, d1..d6, db) " + " ".join("%.1e" % e for e in np.max(worst, 0)))


@pytest.mark.gpu
def test_network_full_size_against_float64_oracle():
    from weaklysuperviseddl_amd.PretrainedBasnetModel import RunInference as ri
    sd = _state_dict()
    u8 = bo.input_u8(2, 256, 256, seed=5)
    x = bo.input_batch(u8)
    net = _dev_net(sd)
    with torch.no_grad():
        ys = net(x.cuda())
    got = torch.stack(ys).cpu().double()
    ref = torch.stack(bo.forward(sd, x))
    errs = (got - ref).abs().reshape(8, -1).max(1).values
    assert errs.max().item() <= 1e-3, errs
    # binarised saliency: norm_pred per image of output #1, > 0.5, outside a band around 0.5
    n_diff = 0
    for b in range(2):
        p_dev = ri.norm_pred(got[0, b]).numpy()
        p_ref = ri.norm_pred(ref[0, b]).numpy()
        band = np.abs(p_ref - 0.5) <= 1e-3
        assert np.array_equal((p_dev > 0.5)[~band], (p_ref > 0.5)[~band])
        n_diff += int(((p_dev > 0.5) != (p_ref > 0.5)).sum())
    report_line(f"BASNet 256x256 B=2 vs float64 oracle: worst error per output {' '.join('%.1e' % e for e in errs)}; "
                f"binarised mask pixels differing (inside the +-1e-3 band): {n_diff} of {2 * 256 * 256}")


@pytest.mark.gpu
def test_maxpool_ceil_bit_exact():
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(0)
    for (B, C, H, W) in ((2, 3, 8, 8), (1, 5, 7, 9), (3, 2, 1, 5), (2, 4, 33, 17)):
        x = torch.randn(B, C, H, W, generator=g)
        x[0, 0, 0, 0] = float("nan")
        got = ops.max_pool_2x2_ceil(x.cuda()).cpu()
        ref = F.max_pool2d(x, 2, 2, ceil_mode=True)
        assert torch.equal(got.nan_to_num(7.0), ref.nan_to_num(7.0)) and got.isnan().equal(ref.isnan()), (B, C, H, W)
    # a channel slice of a wider tensor in, a channel slice out
    big = torch.randn(2, 6, 13, 10, generator=g)
    dst = torch.full((2, 5, 7, 5), -1.0).cuda()
    ops.max_pool_2x2_ceil(big.cuda()[:, 2:5], out=dst[:, 1:4])
    dst = dst.cpu()
    assert torch.equal(dst[:, 1:4], F.max_pool2d(big[:, 2:5], 2, 2, ceil_mode=True))
    assert (dst[:, 0] == -1).all() and (dst[:, 4] == -1).all()


@pytest.mark.gpu
def test_side_output_kernel_against_float64():
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for s, (Cin, h, w) in zip((1, 2, 4, 8, 16, 32), ((64, 32, 24), (64, 16, 16), (128, 8, 12), (256, 4, 4), (512, 2, 3),
                                                     (512, 2, 2))):
        B = 2
        x = torch.relu(torch.randn(B, Cin + 3, h, w, generator=g))[:, 3:]           # a channel slice
        wt = torch.randn(1, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        bias = torch.randn(1, generator=g) * 0.1
        y, lg = ops.side_output(x.cuda(), wt.cuda(), bias.cuda(), s)
        lg64 = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        ref = torch.sigmoid(F.interpolate(lg64, scale_factor=s, mode="bilinear", align_corners=False))
        assert y.shape == (B, 1, h * s, w * s)
        err = (y.cpu().double() - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= 1e-6, (s, err)
        assert (lg.cpu().double() - lg64).abs().max().item() <= 1e-5
        # the up-sample is wsdl_bilinear_fwd's, bit for bit; torch's scale_factor and size paths agree for these s
        up, _ = ops.side_output(x.cuda(), wt.cuda(), bias.cuda(), s, sigmoid=False)
        assert torch.equal(up, ops.bilinear_resize(lg, (h * s, w * s))), s
        l32 = lg.cpu()
        assert torch.equal(F.interpolate(l32, scale_factor=s, mode="bilinear", align_corners=False),
                           F.interpolate(l32, size=(h * s, w * s), mode="bilinear", align_corners=False)), s
    report_line(f"BASNet side-output kernel vs float64 conv+interpolate+sigmoid, s = 1..32: worst {worst:.1e}")


@pytest.mark.gpu
def test_refunet_tail_against_float64():
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(2)
    x = torch.relu(torch.randn(3, 64, 40, 24, generator=g))
    res = torch.randn(3, 1, 40, 24, generator=g)
    wt = torch.randn(1, 64, 3, 3, generator=g) / 24
    bias = torch.randn(1, generator=g)
    y, lg = ops.side_output(x.cuda(), wt.cuda(), bias.cuda(), 1, residual=res.cuda())
    lg64 = F.conv2d(x.double(), wt.double(), bias.double(), padding=1) + res.double()
    assert (lg.cpu().double() - lg64).abs().max().item() <= 1e-5
    assert (y.cpu().double() - torch.sigmoid(lg64)).abs().max().item() <= 1e-6


@pytest.mark.gpu
def test_saliency_quantisation_bit_exact():
    from weaklysuperviseddl_amd.PretrainedBasnetModel import RunInference as ri
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(3)
    d = torch.rand(6, 1, 64, 48, generator=g)
    d[1] = d[1] * 1e-3 + 0.4            # very different ranges per image: a whole-batch min / max shows
    d[2] = d[2] * 50 - 20
    d[3] = 0.7                          # constant image
    d[4, 0, :32] = 0.0
    d[4, 0, 32:] = 1.0
    got = ops.saliency_u8(d.cuda()).cpu().numpy()
    for b in range(6):
        pred = ri.norm_pred(d[b:b + 1, 0]).squeeze().numpy()
        ref = (pred * 255).astype(np.uint8)
        assert np.array_equal(got[b], ref), b


@pytest.mark.gpu
def test_forward_deterministic_and_batch_independent():
    from weaklysuperviseddl_amd import ops
    net = _dev_net()
    x = bo.input_batch(bo.input_u8(2, 64, 96, seed=9)).cuda()
    with torch.no_grad():
        a = torch.stack(net(x))
        b = torch.stack(net(x))
    assert torch.equal(a, b)
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(8, 64, 32, 32, generator=g).relu().cuda()
    wt, bias = (torch.randn(1, 64, 3, 3, generator=g) / 24).cuda(), torch.randn(1, generator=g).cuda()
    res = torch.randn(8, 1, 32, 32, generator=g).cuda()
    y8, l8 = ops.side_output(xs, wt, bias, 4, residual=res)
    y1, l1 = ops.side_output(xs[5:6], wt, bias, 4, residual=res[5:6])
    assert torch.equal(y8[5:6], y1) and torch.equal(l8[5:6], l1)
    assert torch.equal(ops.max_pool_2x2_ceil(xs)[5:6], ops.max_pool_2x2_ceil(xs[5:6]))
    assert torch.equal(ops.saliency_u8(y8)[5:6], ops.saliency_u8(y1))


@pytest.mark.gpu
def test_fast_conv_path_and_no_copies(monkeypatch):
    from weaklysuperviseddl_amd import lib, ops
    net = _dev_net()
    x = torch.randn(1, 3, 256, 256).cuda()
    with torch.no_grad():
        net(x)                                        # layouts / folds cached
    calls = []
    handle = lib()
    real_copy = handle.wsdl_copy_planes
    monkeypatch.setattr(handle, "wsdl_copy_planes", lambda *a: calls.append("copy_planes") or real_copy(*a))
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: calls.append("cat") or real_cat(*a, **k))
    per_conv = []                                     # (Cin, Cout, launch descriptions) of every convolution
    real_conv = ops.conv2d_fwd

    def traced(x_, wf, wshape, *a, **k):
        ops.last_launches()
        y = real_conv(x_, wf, wshape, *a, **k)
        per_conv.append((wshape[1], wshape[0], ops.last_launches()))
        return y
    monkeypatch.setattr(ops, "conv2d_fwd", traced)
    ops.launch_trace(True)
    try:
        with torch.no_grad():
            net(x)
    finally:
        ops.launch_trace(False)
    assert not calls, calls
    assert len(per_conv) == 79, len(per_conv)      # + 7 side outputs and RefUnet's conv_d0 on the single-output kernel = 87
    fast = [(ci, co, t) for ci, co, t in per_conv if ci % 16 == 0 and co % 4 == 0]
    for ci, co, t in fast:
        kinds = [d for d in t.split("; ") if d.startswith(("split<", "fp32_fast<", "fp32_generic<"))]
        assert kinds and all(not d.startswith("fp32_generic") for d in kinds), (ci, co, t)
    report_line(f"BASNet 256x256 forward: {len(per_conv)} conv2d_fwd calls, {len(fast)} with Cin % 16 == 0 and Cout % 4 == 0, "
                f"all on the split / aligned kernels; the other {len(per_conv) - len(fast)} have Cin 3 or 1; "
                "no copy or concat launches")


@pytest.mark.gpu
def test_errors():
    from weaklysuperviseddl_amd import WsdlError
    net = _dev_net()
    with pytest.raises(WsdlError, match="multiples of 32"):
        net(torch.randn(1, 3, 64, 80).cuda())
    with pytest.raises(WsdlError, match="device tensor"):
        net(torch.randn(1, 3, 64, 64))
    net.train()
    with pytest.raises(WsdlError, match="inference only"):
        net(torch.randn(1, 3, 64, 64).cuda())


@pytest.mark.gpu
def test_run_inference_end_to_end(tmp_path):
    from weaklysuperviseddl_amd.PretrainedBasnetModel import RunInference as ri
    from PIL import Image
    from weaklysuperviseddl_amd import ops
    root = tmp_path / "pet"
    (root / "images").mkdir(parents=True)
    (root / "annotations" / "trimaps").mkdir(parents=True)
    names = [f"Cat_{i}" for i in range(3)]
    sizes = [(200, 150), (256, 256), (180, 240)]
    rng = np.random.default_rng(0)
    for i, (n, (w, h)) in enumerate(zip(names, sizes)):
        img = bo.input_u8(1, h, w, seed=50 + i)[0].transpose(1, 2, 0)
        Image.fromarray(img).save(root / "images" / f"{n}.jpg")
        yy, xx = np.mgrid[0:h, 0:w]
        tri = np.where((yy - h / 2) ** 2 + (xx - w / 2) ** 2 < (min(h, w) / 3) ** 2, 1, 2).astype(np.uint8)
        tri[rng.random((h, w)) < 0.05] = 3
        Image.fromarray(tri).save(root / "annotations" / "trimaps" / f"{n}.png")
    (root / "annotations" / "test.txt").write_text("".join(f"{n} 1 1 1\n" for n in names) + "Extra_1 1 1 1\n")
    sd = _state_dict()
    torch.save(sd, tmp_path / "basnet.pth")
    out_dir = tmp_path / "out"
    results, miou, macc = ri.run_inference(str(tmp_path / "basnet.pth"), str(root), str(out_dir), n_images=3, batch_size=2,
                                           verbose=False)
    assert [r[0] for r in results] == names
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import image_to_tensor
    net = _dev_net(sd)
    images = [Image.open(root / "images" / f"{n}.jpg").convert("RGB") for n in names]
    xs = torch.stack([image_to_tensor(im) for im in images])
    with torch.no_grad():                             # the device's own output #1, in run_inference's batches of 2
        d1s = torch.cat([net(xs[i:i + 2].cuda())[0] for i in (0, 2)])
    worst_lvl, flips = 0, 0
    for i, ((n, iou, acc), image) in enumerate(zip(results, images)):
        assert (out_dir / f"{n}_saliency.png").exists()
        x, d1 = xs[i:i + 1], d1s[i:i + 1]
        u8 = ops.saliency_u8(d1).cpu().numpy()[0]
        pred = np.array(Image.fromarray(u8).resize(image.size)) / 255.0
        gt = np.array(Image.open(root / "annotations" / "trimaps" / f"{n}.png").resize(image.size, resample=Image.NEAREST))
        iou2, acc2, _, _ = ri.compute_metrics(pred, gt)
        assert iou == iou2 and acc == acc2, n
        assert np.array_equal(np.array(Image.open(out_dir / f"{n}_saliency.png")), (pred * 255).round().astype(np.uint8))
        # against the float64 oracle's output #1, quantised the reference's way
        o1 = bo.forward(sd, x)[0][0, 0]
        ref_u8 = (ri.norm_pred(o1).numpy() * 255).astype(np.uint8)
        assert (d1.cpu().double()[0, 0] - o1).abs().max().item() <= 1e-3
        lvl = np.abs(u8.astype(int) - ref_u8.astype(int))
        worst_lvl = max(worst_lvl, int(lvl.max()))
        flips += int((lvl > 0).sum())
        assert lvl.max() <= 1
    assert miou == pytest.approx(np.mean([r[1] for r in results])) and macc == pytest.approx(np.mean([r[2] for r in results]))
    report_line(f"BASNet run_inference on 3 synthetic Pet images: mean IoU {miou:.4f}, acc {macc:.4f}; uint8 saliency vs "
                f"float64 oracle: {flips} pixels one level apart (max {worst_lvl})")
