"""Pixel-adaptive mask refinement on the device (csrc/pamr.hip) against the float64 oracle of tests/pamr_oracle.py.

Parity bound: the SAME oracle run in torch float32 on the CPU against its float64 run is the yardstick, computed here per
case; the device may be at most 4 x that (a different summation order over up to 48 terms and a different ``exp``; the errors
do not grow geometrically with the iterations because every iteration is a convex combination).  The worst device values are
reported with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pamr_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs, the float64 oracle and the float32 yardstick of one case - computed once, shared, never written."""
    B, H, W, C, K, dil = po.CASES[case]
    img, m = po.make_inputs(B, H, W, C, K, 10 + case)
    w64 = po.affinity(img, dil)
    out64 = po.propagate(w64, m, 10, dil)
    w32 = po.affinity(img, dil, dtype=torch.float32)
    out32 = po.propagate(w32, m, 10, dil)
    assert w32.dtype == torch.float32 and out32.dtype == torch.float32
    yard_w = (w32.double() - w64).abs().max().item()
    yard_m = (out32.double() - out64).abs().max().item()
    return dict(img=img, m=m, dil=dil, w64=w64, out64=out64, yard_w=yard_w, yard_m=yard_m)


def maxerr(a, b):
    return (a.detach().cpu().double() - b).abs().max().item()


@pytest.mark.parametrize("case", range(len(po.CASES)))
def test_weights_and_refined_scores_against_float64(dev, case):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = reference(case)
    x, m = r["img"].to(dev), r["m"].to(dev)
    w = ops.pamr_affinity(x, r["dil"])
    out = ops.pamr(x, m, 10, r["dil"])
    e_w, e_m = maxerr(w, r["w64"]), maxerr(out, r["out64"])
    shape = "x".join(str(v) for v in po.CASES[case][:5])
    report_line(f"pamr {shape} D={len(r['dil'])}: max |device - float64| weights {e_w:.2e} (float32 oracle {r['yard_w']:.2e}), "
                f"scores after 10 iterations {e_m:.2e} (float32 oracle {r['yard_m']:.2e})")
    print(f"case {case}: weights {e_w:.3e} / yardstick {r['yard_w']:.3e}; scores {e_m:.3e} / yardstick {r['yard_m']:.3e}; "
          f"oracle output spans {r['out64'].min().item():.3f} .. {r['out64'].max().item():.3f}")
    assert tuple(w.shape) == tuple(r["w64"].shape) and w.dtype == torch.float32 and w.is_contiguous()
    assert out.dtype == torch.float32 and out.grad_fn is None and not out.requires_grad
    assert (w.sum(dim=1) - 1).abs().max().item() < 1e-6
    assert e_w <= 4 * r["yard_w"], (e_w, r["yard_w"])
    assert e_m <= 4 * r["yard_m"], (e_m, r["yard_m"])
    # a convex combination: inside the input's range; a constant map is a fixed point
    assert out.min().item() >= m.min().item() - 1e-6 and out.max().item() <= m.max().item() + 1e-6
    const = torch.full_like(m, 0.625)
    assert (ops.pamr(x, const, 10, r["dil"], affinity=w) - 0.625).abs().max().item() < 1e-6


def test_flat_image_gives_uniform_weights(dev):
    from weaklysuperviseddl_amd import ops
    w = ops.pamr_affinity(torch.full((1, 3, 9, 70), 0.37, device=dev))
    assert torch.equal(w, torch.full_like(w, 1.0 / 48))


@pytest.mark.parametrize("case", (1, 2))
def test_bit_identical_paths(dev, case):
    """A given affinity, split iteration counts, every parity of num_iter into ``out``, and a second run: the same bits."""
    from weaklysuperviseddl_amd import ops
    r = reference(case)
    x, m, dil = r["img"].to(dev), r["m"].to(dev), r["dil"]
    m0 = m.clone()
    full = ops.pamr(x, m, 7, dil)
    w = ops.pamr_affinity(x, dil)
    assert torch.equal(ops.pamr(x, m, 7, dil, affinity=w), full)
    assert torch.equal(ops.pamr(x, ops.pamr(x, m, 3, dil), 4, dil), full)
    assert torch.equal(ops.pamr(x, m, 7, dil), full)
    prev = m
    for n in (0, 1, 2, 3):
        o = torch.full_like(m, float("nan"))
        got = ops.pamr(x, m, n, dil, affinity=w, out=o)
        assert got is o and not torch.isnan(o).any()
        if n == 0:
            assert torch.equal(o, m)
        else:
            assert torch.equal(o, ops.pamr(x, prev, 1, dil, affinity=w)), n
        prev = o
    assert torch.equal(m, m0)                                     # the input is never written
    # a strided view of the scores (channel slice of a wider tensor) and requires_grad inputs are accepted, detached
    wide = torch.cat([m, m], dim=1)[:, 1:1 + m.shape[1]].requires_grad_()
    res = ops.pamr(x, wide, 2, dil)
    assert res.grad_fn is None and torch.equal(res, ops.pamr(x, wide.detach().contiguous(), 2, dil))


def test_refusals_on_the_device(dev):
    from weaklysuperviseddl_amd import ops
    x, m = torch.rand(1, 3, 8, 8, device=dev), torch.rand(1, 2, 8, 8, device=dev)
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, torch.rand(1, 2, 8, 9, device=dev))           # another size
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, torch.rand(2, 2, 8, 8, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, m, out=m)                                     # aliasing
    with pytest.raises(ops.WsdlError):
        ops.pamr(torch.rand(1, 5, 8, 8, device=dev), m)
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, torch.rand(1, 33, 8, 8, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, m, affinity=torch.rand(1, 40, 8, 8, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.pamr(x.double(), m)


def test_many_score_channels_take_several_launches_per_iteration(dev):
    """C = 7: a group of four and a group of three per iteration; each channel equals its own one-channel run."""
    from weaklysuperviseddl_amd import ops
    r = reference(1)
    x, dil = r["img"].to(dev), r["dil"]
    g = torch.Generator().manual_seed(5)
    m = torch.rand(2, 7, 37, 53, generator=g).to(dev)
    w = ops.pamr_affinity(x, dil)
    out = ops.pamr(x, m, 3, dil, affinity=w)
    for c in range(7):
        assert torch.equal(out[:, c:c + 1], ops.pamr(x, m[:, c:c + 1], 3, dil, affinity=w)), c


@pytest.mark.parametrize("case", range(len(po.CASES)))
def test_labels_against_the_oracle(dev, case):
    """Compared where the float64 margin to a decision boundary is at least 10 x the parity bound; at most 1 % left out."""
    from weaklysuperviseddl_amd import ops
    r = reference(case)
    out = ops.pamr(r["img"].to(dev), r["m"].to(dev), 10, r["dil"])
    thresh, min_conf = 0.3, 0.4
    got = ops.pamr_labels(out, thresh=thresh, min_conf=min_conf, ignore_index=255).cpu()
    want = po.labels(r["out64"], thresh, min_conf, 255)
    sure = po.label_margin(r["out64"], thresh, min_conf) >= 10 * 4 * r["yard_m"]
    assert got.dtype == torch.int64 and tuple(got.shape) == tuple(want.shape)
    assert (~sure).double().mean().item() <= 0.01
    assert torch.equal(got[sure], want[sure])
    assert len(torch.unique(want)) >= 2                          # (the case decides something)


def test_labels_ties_and_boundaries(dev):
    from weaklysuperviseddl_amd import ops
    s = torch.tensor([[0.2, 0.7, 0.7, 0.1], [0.3, 0.1, 0.3, 0.3], [0.9, 0.1, 0.0, 0.95]], device=dev).t().reshape(1, 4, 1, 3).contiguous()
    assert ops.pamr_labels(s).flatten().tolist() == [1, 0, 3]                      # equal channels: the lower index
    assert ops.pamr_labels(s, min_conf=0.7).flatten().tolist() == [1, 255, 3]      # maximum == min_conf: kept
    assert ops.pamr_labels(s, min_conf=0.75, ignore_index=-100).flatten().tolist() == [-100, -100, 3]
    one = torch.tensor([0.5, 0.4999, 0.6, 0.0], device=dev).view(1, 1, 2, 2)
    assert ops.pamr_labels(one, thresh=0.5).flatten().tolist() == [1, 0, 1, 0]     # m == thresh: foreground
    assert ops.pamr_labels(one, thresh=0.5, min_conf=0.9).flatten().tolist() == [1, 0, 1, 0]


def test_a_launch_plan_replays_the_call(dev):
    from weaklysuperviseddl_amd import ops, plan
    r = reference(1)
    x, m = r["img"].to(dev), r["m"].to(dev)
    o = torch.empty_like(m)
    p, res = plan.record(ops.pamr, x, m, out=o)
    assert res is o and p.stats["kernels"] == 11 and torch.equal(o, ops.pamr(x, m))
    # new contents in the same buffers
    x2 = (x * 0.5 + 0.25 * x.flip(-1)).contiguous()
    m2 = (1 - m).contiguous()
    x.copy_(x2)
    m.copy_(m2)
    p.replay()
    torch.cuda.synchronize()
    replayed = o.clone()
    assert torch.equal(replayed, ops.pamr(x2.clone(), m2.clone())) and not torch.equal(replayed, ops.pamr(r["img"].to(dev), r["m"].to(dev)))


def test_module_and_callers(dev):
    """wnn.PAMR is ops.pamr; refine_dataset(method="pamr") equals pamr applied by hand; generate_pseudo_masks(pamr=None) is
    the call without the argument, bit for bit, and pamr={} changes the masks through the documented composition."""
    from conftest import smooth_image
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import (InMemoryPseudoDataset, build_segmentation_model, refine_dataset)
    from weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss import network_soft_prediction
    r = reference(1)
    x, m = r["img"].to(dev), r["m"].to(dev)
    assert torch.equal(wnn.PAMR(4, (1, 2))(x, m), ops.pamr(x, m, 4, (1, 2)))

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
    ds = InMemoryPseudoDataset(((img - mean) / std).to(dev), masks.to(dev))
    S = network_soft_prediction(model, ds.images)
    thr = S[:, 1].median().item()                                 # (a threshold that splits the toy prediction)
    want = (ops.pamr(ds.images, S, 5, (1, 2, 4))[:, 1] > thr).to(torch.uint8) * 255
    refine_dataset(model, ds, repeats=3, chunk=4, threshold=thr, method="pamr", pamr_kwargs=dict(num_iter=5, dilations=(1, 2, 4)))
    assert torch.equal(ds.masks, want) and 0 < int((want > 0).sum()) < want.numel()


def test_generate_pseudo_masks_without_pamr_is_unchanged(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM, LayerCAMGenerator, generate_pseudo_masks
    torch.manual_seed(0)
    model = FrozenResNetCAM(37)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    gen = LayerCAMGenerator(model.to(dev).eval(), ["layer3", "layer4"])
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 224, 224, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_pseudo_masks(loader, gen, pamr=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    # pamr={}: the CAM without its threshold, refined as one channel, thresholded, keep_largest
    generate_pseudo_masks(loader, gen, pamr={}, **kw)
    refined = torch.stack(generate_pseudo_masks.last_masks)
    imgs = loader[0][0].to(dev)
    cam, _ = gen.generate_batch(imgs, alpha=1.0, class_idx=loader[0][1][0].to(dev), thresh=0.3)
    want = ops.keep_largest_batched(ops.pamr_labels(ops.pamr(imgs, cam[:, None]), thresh=0.3).to(torch.uint8))
    assert torch.equal(refined, want) and refined.dtype == torch.uint8
