"""Signed distance maps, the fused boundary loss (Kervadec et al., MIDL 2019), its two criteria, a planned training step with
them, and the surface-distance statistics / metrics on the device (csrc/boundary_loss.hip) against the oracle of
tests/boundary_loss_oracle.py.

Parity bound of the loss and the gradient: the SAME oracle run in torch float32 on the CPU against its float64 run is the
yardstick, computed here per case; the device may be at most 4 x that (the margin of tests/test_hip_edt.py and
tests/test_hip_pamr.py).  Where the yardstick is 0 - an image without a contour: every phi is 0 - the bound is 2^-22 times the
largest magnitude compared.  Distances, counts, maxima and percentiles are integers: equal, never close.  ``sum_d`` is a sum of
non-negative doubles: any order is within n 2^-52 relative of the exact sum.  The worst device values are reported with
``report_line``."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_loss_oracle as bo  # noqa: E402
import edt_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu

IGNORE = 255
COMBOS = [(C, cl) for C in bo.CHANNELS for cl in bo.CLASS_LISTS if max(cl) < C]          # (2, 0) needs C >= 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case_labels(case):
    B, H, W = bo.CASES[case]
    return eo.make_labels(B, H, W, 700 + case)


@functools.lru_cache(maxsize=None)
def planes(case, value):
    """The oracle's integer planes (border=False) of one class of one case - computed once, shared, never written.  The
    all-pairs oracle up to 64 x 64; above, its axis-by-axis form (equal: tests/test_boundary_loss.py), which takes
    milliseconds where the former takes seconds."""
    B, H, W = bo.CASES[case]
    return eo.dist2(case_labels(case), value, "euclid", False) if H * W <= 4096 else bo.dist2_separable(case_labels(case), value)


@functools.lru_cache(maxsize=None)
def phi_ref(case, value, dtype=torch.float64):
    return bo.signed_distance(case_labels(case), value, dtype, planes=planes(case, value))


def phi_classes(case, classes, dtype):
    return torch.stack([phi_ref(case, c, dtype) for c in classes], dim=1)


def ulps(a, b):
    """The distance of two float32 tensors in units of the last place of the larger magnitude."""
    a, b = a.double(), b.double()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    return ((a - b).abs() / torch.exp2(torch.floor(torch.log2(mag)) - 23)).max().item()


# ------------------------------------------------------------------------------------------------------ 1. signed distance
@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_signed_distance_recovers_the_planes_and_equals_float64(dev, case):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    labels = case_labels(case)
    worst = 0.0
    for value in (1, 0, 2):
        d_out, d_in = planes(case, value)
        phi = ops.signed_distance(labels.to(dev), value)
        assert phi.dtype == torch.float32 and tuple(phi.shape) == tuple(labels.shape) and phi.is_contiguous()
        got = phi.cpu()
        inside = labels == value
        flat = ((d_out >= eo.FAR) | (d_in >= eo.FAR)).flatten(1).any(dim=1)
        for b in range(labels.shape[0]):
            if flat[b]:
                assert (got[b] == 0).all(), (value, b)                  # the class is absent from the image or fills it
                continue
            # phi^2 recovers the integer planes
            assert torch.equal((got[b].double() ** 2).round().long()[~inside[b]], d_in[b][~inside[b]]), (value, b)
            assert torch.equal(((1.0 - got[b].double()) ** 2).round().long()[inside[b]], d_out[b][inside[b]]), (value, b)
            assert (got[b][~inside[b]] >= 1).all() and (got[b][inside[b]] <= 0).all()
        want = phi_ref(case, value, torch.float32)
        worst = max(worst, ulps(got, want))
    shape = "x".join(str(v) for v in bo.CASES[case])
    report_line(f"signed distance {shape}: worst |device - float32(float64 formula)| {worst:.2f} ulp")
    assert worst <= 1.0, worst
    assert (labels == IGNORE).sum() == 0 or (ops.signed_distance(labels.to(dev), 1).cpu()[labels == IGNORE] >= 0).all()


def test_signed_distance_special_images_void_pixels_and_buffers(dev):
    from weaklysuperviseddl_amd import ops
    labels = case_labels(3).clone()
    labels[1] = 1                                                        # full
    labels[2][labels[2] == 1] = 0                                        # absent
    on_dev = labels.to(dev)
    bufs = {}
    phi = ops.signed_distance(on_dev, out=bufs)
    assert phi is bufs["phi"] and bufs["out"].dtype == torch.int32 and bufs["in"].dtype == torch.int32
    assert (phi[1] == 0).all() and (phi[2] == 0).all() and (phi[0] != 0).any()
    assert torch.equal(phi[0].cpu(), phi_ref(3, 1, torch.float32)[0])
    void = labels[0] == IGNORE
    assert void.any() and (phi[0].cpu()[void] >= 1).all()                # void pixels are OUT
    ptrs = [bufs[k].data_ptr() for k in ("phi", "out", "in")]
    first = phi.clone()
    again = ops.signed_distance(on_dev, out=bufs)
    assert [bufs[k].data_ptr() for k in ("phi", "out", "in")] == ptrs and again is bufs["phi"] and torch.equal(again, first)
    assert torch.equal(ops.signed_distance((labels == 1).to(dev)), first)                 # a bool mask is converted
    with pytest.raises(ops.WsdlError):
        ops.signed_distance(torch.zeros(4, 4, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("case,classes", ((3, (1,)), (3, (2, 0)), (5, (0, 1)), (2, (2, 0, 1)), (0, (1, 0))))
def test_signed_distance_classes_equals_the_per_class_calls(dev, case, classes):
    from weaklysuperviseddl_amd import ops
    on_dev = case_labels(case).to(dev)
    bufs = {}
    phi = ops.signed_distance_classes(on_dev, classes, out=bufs)
    B, H, W = bo.CASES[case]
    assert phi.dtype == torch.float32 and tuple(phi.shape) == (B, len(classes), H, W) and phi.is_contiguous() and phi is bufs["phi"]
    for k, c in enumerate(classes):
        assert torch.equal(phi[:, k], ops.signed_distance(on_dev, c)), (k, c)
    ptr = phi.data_ptr()
    assert ops.signed_distance_classes(on_dev, classes, out=bufs).data_ptr() == ptr


# ------------------------------------------------------------------------------------------------------ 2. loss and gradient
def device_loss_and_grad(dev, logits, phi, labels, **kw):
    from weaklysuperviseddl_amd import ops
    z = logits.to(dev).requires_grad_()
    loss = ops.boundary_loss(z, phi.to(dev), None if labels is None else labels.to(dev), **kw)
    loss.backward()
    return loss.detach().cpu(), z.grad.cpu()


def bound(yard, *compared):
    return 4 * yard if yard > 0 else 2.0 ** -22 * max(float(t.abs().max()) for t in compared)


@pytest.mark.parametrize("C,classes", COMBOS)
@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_loss_and_gradient_against_float64(dev, case, C, classes):
    from conftest import report_line
    B, H, W = bo.CASES[case]
    labels = case_labels(case)
    logits = bo.make_logits(B, C, H, W, 900 + case)
    phi32 = phi_classes(case, classes, torch.float32)
    l64, g64 = bo.loss_and_grad(logits, phi32, labels, classes, IGNORE)
    l32, g32 = bo.loss_and_grad(logits, phi32, labels, classes, IGNORE, dtype=torch.float32)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32
    yard_l = abs(float(l32) - float(l64))
    yard_g = (g32.double() - g64).abs().max().item()
    loss, grad = device_loss_and_grad(dev, logits, phi32, labels, classes=classes, ignore_index=IGNORE)
    err_l = abs(float(loss) - float(l64))
    err_g = (grad.double() - g64).abs().max().item()
    shape = "x".join(str(v) for v in bo.CASES[case])
    print(f"boundary loss {shape} C={C} classes={classes}: loss {float(l64):+.6e}, device error {err_l:.3e} (float32 oracle "
          f"{yard_l:.3e}); gradient max {g64.abs().max().item():.3e}, device error {err_g:.3e} (float32 oracle {yard_g:.3e})")
    report_line(f"boundary loss {shape} C={C} classes={classes}: |device - float64| loss {err_l:.2e} (float32 oracle {yard_l:.2e}), "
                f"gradient {err_g:.2e} (float32 oracle {yard_g:.2e})")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32 and tuple(grad.shape) == (B, C, H, W)
    assert err_l <= bound(yard_l, l64), (err_l, yard_l)
    assert err_g <= bound(yard_g, g64), (err_g, yard_g)
    assert (grad.permute(0, 2, 3, 1)[labels == IGNORE] == 0).all()       # invalid pixels: exactly 0


# ------------------------------------------------------------------------------------------------------ 3. special cases
def test_no_valid_pixel_gives_zero_not_nan(dev):
    labels = torch.full((2, 37, 53), IGNORE, dtype=torch.int64)
    logits = bo.make_logits(2, 3, 37, 53, 1)
    phi = phi_classes(3, (1, 0), torch.float32)[:2]
    loss, grad = device_loss_and_grad(dev, logits, phi, labels, classes=(1, 0), ignore_index=IGNORE)
    assert float(loss) == 0.0 and not grad.any() and torch.isfinite(grad).all()


@pytest.mark.parametrize("case", (3, 4))
def test_labels_none_phi_rank_three_and_unlisted_classes(dev, case):
    B, H, W = bo.CASES[case]
    labels = case_labels(case)
    logits = bo.make_logits(B, 3, H, W, 5)
    phi = phi_classes(case, (1,), torch.float32)
    # labels=None equals labels without an ignored pixel, bit for bit
    l_none, g_none = device_loss_and_grad(dev, logits, phi, None, classes=(1,))
    l_lab, g_lab = device_loss_and_grad(dev, logits, phi, labels, classes=(1,), ignore_index=-100)
    assert torch.equal(l_none, l_lab) and torch.equal(g_none, g_lab) and g_none.abs().sum() > 0
    # phi (B,H,W) equals (B,1,H,W)
    l3, g3 = device_loss_and_grad(dev, logits, phi[:, 0].contiguous(), None, classes=(1,))
    assert torch.equal(l3, l_none) and torch.equal(g3, g_none)
    # a class outside `classes` contributes through the softmax only: its plane may hold anything when it is listed with
    # phi = 0, and raising its logit changes the loss only by shrinking the listed probabilities
    two = torch.cat([phi, torch.zeros_like(phi)], dim=1)
    l2, g2 = device_loss_and_grad(dev, logits, two, None, classes=(1, 2))
    assert abs(float(l2) * 2 - float(l_none)) <= 2.0 ** -22 * abs(float(l_none))
    assert ((g2 * 2).double() - g_none.double()).abs().max().item() <= 2.0 ** -22 * g_none.abs().max().item()
    l64, g64 = bo.loss_and_grad(logits, phi, None, (1,))
    assert (g64[:, 0] + g64[:, 1] + g64[:, 2]).abs().max().item() <= 1e-17          # softmax gradients sum to 0 over C
    assert (g_none.double().sum(dim=1)).abs().max().item() <= 3 * 2.0 ** -23 * g_none.abs().max().item()


def test_scale_on_the_device_equals_the_scaled_result(dev):
    """loss = float32(scale S / (K N)) against float32(S / (K N)) * scale: within 1 ulp.  The gradient is dl * float32(g *
    inv): with the scale inside ``inv`` that is two roundings (inv, the product), multiplied afterwards three (inv, two
    products) - five roundings of at most 2^-24 relative each between the two results."""
    from weaklysuperviseddl_amd import ops
    B, H, W = bo.CASES[3]
    logits = bo.make_logits(B, 2, H, W, 8)
    phi = phi_classes(3, (1,), torch.float32)
    labels = case_labels(3)
    l1, g1 = device_loss_and_grad(dev, logits, phi, labels, classes=(1,), ignore_index=IGNORE)
    scale = torch.tensor([0.37], dtype=torch.float32, device=dev)
    ls, gs = device_loss_and_grad(dev, logits, phi, labels, classes=(1,), ignore_index=IGNORE, scale=scale)
    s32 = torch.tensor(0.37, dtype=torch.float32)
    assert float(l1) != 0 and ulps(ls, l1 * s32) <= 1.0
    assert ((gs.double() - (g1 * s32).double()).abs() <= 5 * 2.0 ** -24 * gs.double().abs()).all() and gs.abs().sum() > 0
    scale.fill_(2.0)                                                     # a power of two: exact
    l2, g2 = device_loss_and_grad(dev, logits, phi, labels, classes=(1,), ignore_index=IGNORE, scale=scale)
    assert torch.equal(l2, l1 * 2) and torch.equal(g2, g1 * 2)
    with pytest.raises(ops.WsdlError):
        ops.boundary_loss(logits.to(dev), phi.to(dev), scale=torch.ones(2, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.boundary_loss(logits.to(dev), phi.to(dev)[:, :, :5])


@pytest.mark.parametrize("classes,C", (((1,), 2), ((2, 0), 3)))
def test_boundary_loss_module_equals_the_ops(dev, classes, C):
    from weaklysuperviseddl_amd import ops, nn as wnn
    B, H, W = bo.CASES[3]
    labels = case_labels(3).to(dev)
    logits = bo.make_logits(B, C, H, W, 12).to(dev)
    crit = wnn.BoundaryLoss(classes, ignore_index=IGNORE)
    za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    la = crit(za, labels)
    lb = ops.boundary_loss(zb, ops.signed_distance_classes(labels, classes), labels, classes=classes, ignore_index=IGNORE)
    la.backward()
    lb.backward()
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0
    # the buffers keep their addresses from call to call and move with the shape
    ptrs = (crit.phi_ptr, crit.d2_out_ptr, crit.d2_in_ptr)
    crit(za.detach(), labels)
    assert ptrs == (crit.phi_ptr, crit.d2_out_ptr, crit.d2_in_ptr) == (crit.phi.data_ptr(), crit.d2_out.data_ptr(), crit.d2_in.data_ptr())
    crit(za.detach()[:, :, :20].contiguous(), labels[:, :20].contiguous())
    assert tuple(crit.phi.shape) == (B, len(classes), 20, W) and crit.phi_shape == f"{B}x{len(classes)}x20x{W}"


@pytest.mark.parametrize("weighted", (False, True))
def test_alpha_zero_is_the_cross_entropy_bit_for_bit(dev, weighted):
    from weaklysuperviseddl_amd import nn as wnn
    B, H, W = bo.CASES[3]
    labels = (case_labels(3) == 1).long()
    kw = {}
    if weighted:
        labels[:, 5:9, 30:40] = IGNORE
        kw = dict(weight=torch.tensor([0.7, 1.9]), ignore_index=IGNORE, label_smoothing=0.1)
    labels = labels.to(dev)
    logits = bo.make_logits(B, 2, H, W, 13).to(dev)
    crit = wnn.CrossEntropyBoundaryLoss(alpha=0.0, **kw).to(dev)
    ref = wnn.CrossEntropyLoss(**kw).to(dev)
    za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    la, lb = crit(za, labels), ref(zb, labels)
    la.backward()
    lb.backward()
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0
    # with alpha > 0 it is the sum of the two terms
    crit.set_alpha(0.25)
    zc, zd = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    lc = crit(zc, labels)
    bl = wnn.BoundaryLoss(ignore_index=kw.get("ignore_index", -100))(zd, labels)
    lc, lb, bl = lc.item(), lb.item(), bl.item()
    assert lc != lb and abs(lc - (lb + 0.25 * bl)) <= 2.0 ** -22 * (abs(lb) + abs(bl))


# ------------------------------------------------------------------------------------------------------ 4. launch plan
def test_planned_step_replays_through_an_alpha_schedule_and_records_anew_for_other_classes(dev):
    """Ten steps on the smallest configuration of tests/test_hip_plan.py (the reference's model, 4 x 64 x 64), two batches with
    different masks in turn: eager, eager, record (+ verification on a probe batch), replay; then ``set_alpha`` - the SAME plan
    replays three more times; then ``classes`` change: eager (a key seen once), record, replay.  Every loss and the final state
    equal the eager run's bit for bit; a run that keeps the old alpha - what a plan with a frozen alpha would compute - has
    another loss at step 5."""
    from weaklysuperviseddl_amd import plan, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(4, 3, 64, 64, generator=g).to(dev), (eo.make_labels(4, 64, 64, 70 + i) == 1).long().to(dev))
               for i in range(2)]
    assert not torch.equal(batches[0][1], batches[1][1])

    def run(planned, schedule):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = build_segmentation_model().to(dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = wnn.CrossEntropyBoundaryLoss(alpha=schedule[0][0], classes=schedule[0][1]).to(dev)
            torch.manual_seed(1234)
            losses, plans = [], []
            for i, (alpha, classes) in enumerate(schedule):
                crit.set_alpha(alpha)
                crit.boundary.set_classes(classes)
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
                st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
                plans.append(None if st is None else (id(st), st.records, st.replays))
            torch.cuda.synchronize()
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st, plans
        finally:
            plan.PLAN_STEP[0] = old

    schedule = [(0.01, (1,))] * 4 + [(0.5, (1,))] * 3 + [(0.5, (0,))] * 3
    l0, s0, _, _ = run(False, schedule)
    l1, s1, st, plans = run(True, schedule)
    stale, _, _, _ = run(False, [(0.01, (1,))] * 5)
    print(f"planned boundary-loss step: losses {l1}, records {st.records}, replays {st.replays}; step 5 with the old alpha {stale[4]}")
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert plans[3][1:] == (1, 1) and plans[6][1:] == (1, 4), plans      # after set_alpha: the same plan, no new recording
    assert len({p[0] for p in plans if p is not None}) == 1
    assert st.records == 2 and st.replays == 5, (st.records, st.replays)  # other classes: a new plan
    assert l0 == l1 and all(v == v for v in l0), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert stale[:4] == l0[:4] and stale[4] != l0[4]


# ------------------------------------------------------------------------------------------------------ 5. surface stats
def stats_batch():
    """(8,37,53): two blob images against shifted / other blobs; identical masks; an empty prediction; an empty ground truth;
    both empty; one pixel each; a mask that touches the image edge."""
    labels = eo.make_labels(8, 37, 53, 41)
    preds = eo.make_labels(8, 37, 53, 42)
    preds[0] = torch.roll(labels[0], (2, -3), (0, 1))
    preds[2] = labels[2]
    preds[3][preds[3] == 1] = 0
    labels[4][labels[4] == 1] = 2
    preds[5].zero_()
    labels[5].zero_()
    preds[6].zero_()
    labels[6].zero_()
    preds[6, 3, 50] = 1
    labels[6, 30, 4] = 1
    preds[7].zero_()
    labels[7].zero_()
    preds[7, 0:9, 0:53] = 1
    labels[7, 20:37, 40:53] = 1
    return preds, labels


def check_stats(got, want):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got["n"].dtype == np.int64 and got["max_d2"].dtype == np.int32 and got["sum_d"].dtype == np.float64
    assert got["pct_d2"].dtype == np.float32
    assert np.array_equal(got["n"], want["n"]), (got["n"], want["n"])
    assert np.array_equal(got["max_d2"].astype(np.int64), want["max_d2"])
    assert np.array_equal(got["pct_d2"].astype(np.float64), want["pct_d2"]), (got["pct_d2"], want["pct_d2"])
    rel = np.abs(got["sum_d"] - want["sum_d"]) / np.maximum(want["sum_d"], 1e-300)
    assert (rel <= np.maximum(want["n"], 1) * 2.0 ** -52).all(), rel
    return got, float(rel.max())


@pytest.mark.parametrize("percentile", (95.0, 100.0, 50.0))
def test_surface_stats_are_exact(dev, percentile):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    preds, labels = stats_batch()
    want = bo.surface_stats(preds, labels, 1, percentile)
    got, rel = check_stats(ops.surface_distance_stats(preds.to(dev), labels.to(dev), percentile=percentile), want)
    report_line(f"surface stats 8x37x53 percentile {percentile}: n, max_d2, pct_d2 exact; sum_d within {rel:.1e} relative")
    assert tuple(got["n"].shape) == (8, 2)
    assert (got["n"][2] > 0).all() and not got["max_d2"][2].any() and not got["sum_d"][2].any() and not got["pct_d2"][2].any()
    assert got["n"][3, 0] == 0 and got["n"][3, 1] > 0 and got["n"][4, 1] == 0 and got["n"][4, 0] > 0 and not got["n"][5].any()
    assert got["n"][6].tolist() == [1, 1] and got["max_d2"][6].tolist() == [27 ** 2 + 46 ** 2] * 2
    assert got["n"][7, 0] == 2 * 53 + 2 * 7                              # the image edge counts as surface: the ring of a 9 x 53 block
    if percentile == 100.0:
        assert np.array_equal(got["pct_d2"][got["n"] > 0], got["max_d2"][got["n"] > 0].astype(np.float32))
    # the host function: nan where a surface is empty, the oracle's metrics elsewhere
    per, means, defined = ops.surface_distances_from_stats(got)
    want_per, want_means, want_defined = bo.metrics(want)
    assert defined == want_defined == 5 and all(math.isnan(per[i]["hd"]) and math.isnan(per[i]["assd"]) for i in (3, 4, 5))
    for p, w in zip(per, want_per):
        for key in ("hd", "hd95", "assd"):
            assert (math.isnan(p[key]) and math.isnan(w[key])) or abs(p[key] - w[key]) <= 1e-12 * max(1.0, w[key]), (key, p, w)
    assert all(abs(means[k] - want_means[k]) <= 1e-12 * want_means[k] for k in means)
    per2, means2, defined2 = ops.surface_distances(preds.to(dev), labels.to(dev), percentile=percentile)
    assert defined2 == defined and means2 == means


@pytest.mark.parametrize("case", (2, 4, 6))
def test_surface_stats_on_other_shapes_buffers_and_run_to_run(dev, case):
    from weaklysuperviseddl_amd import ops
    B, H, W = bo.CASES[case]
    labels = eo.make_labels(B, H, W, 43 + case)
    preds = torch.roll(labels, (1, 2), (1, 2))
    want = bo.surface_stats(preds, labels, 1, 95.0)
    bufs = {}
    first = ops.surface_distance_stats(preds.to(dev), labels.to(dev), out=bufs)
    got, _ = check_stats(first, want)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    again = ops.surface_distance_stats(preds.to(dev), labels.to(dev), out=bufs)
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    assert all(np.array_equal(again[k].cpu().numpy(), got[k]) for k in got)              # bitwise reproducible, sum_d included
    same = ops.surface_distance_stats(labels.to(dev), labels.to(dev))
    assert not same["max_d2"].any() and not same["sum_d"].any() and not same["pct_d2"][same["n"] > 0].any()
    assert torch.equal(same["n"][:, 0], same["n"][:, 1])
    # another class
    check_stats(ops.surface_distance_stats(preds.to(dev), labels.to(dev), 2), bo.surface_stats(preds, labels, 2, 95.0))


def test_surface_stats_refuse_sides_whose_squares_leave_float32(dev):
    from weaklysuperviseddl_amd import ops
    tall = torch.ones(1, 4096, 1, dtype=torch.int64, device=dev)         # 4096^2 + 1 >= 2^24
    with pytest.raises(ops.WsdlError):
        ops.surface_distance_stats(tall, tall)
    ok = torch.ones(1, 4095, 1, dtype=torch.int64, device=dev)           # 4095^2 + 1 < 2^24
    st = ops.surface_distance_stats(ok, ok)
    assert st["n"].tolist() == [[4095, 4095]] and not st["max_d2"].any()
    with pytest.raises(ops.WsdlError):
        ops.surface_distance_stats(ok, ok[:, :10])


# ------------------------------------------------------------------------------------------------------ 6. evaluation
def test_evaluate_surface_distances_equals_the_oracle(dev):
    """A stub model whose logits come from a table keyed on the image's first value; three batches, the first image of each
    counts, one of them with a ground truth of another size (nearest resize of the prediction), one with an empty prediction
    (left out of the means)."""
    from weaklysuperviseddl_amd.TraditionalModel import evaluate_surface_distances

    preds = (eo.make_labels(3, 37, 53, 81) == 1).long()
    preds[2].zero_()

    class Stub(torch.nn.Module):
        def forward(self, x):
            p = preds[int(x[0, 0, 0, 0].item())].to(x.device)
            return {"out": torch.stack([1.0 - p.float(), p.float()])[None]}

    def image(i):
        return torch.full((2, 3, 37, 53), float(i))

    tri0 = torch.where(torch.roll(preds[0], (1, -2), (0, 1)) == 1, 1, 2)
    tri0[0:3, 0:9] = 3
    tri1 = torch.where(eo.make_labels(1, 50, 40, 82)[0] == 1, 1, 2)
    tri2 = tri0.clone()

    for binarize in ("notebook", "modular"):
        shift = 1 if binarize == "notebook" else 0
        loader = [(image(i), (torch.zeros(2), torch.stack([t - shift, t - shift]))) for i, t in enumerate((tri0, tri1, tri2))]
        stats = []
        for (img, (_l, tm)), p in zip(loader, preds):
            gt = tm[0].clone()
            if binarize == "notebook":
                gt[gt == 2] = 1
                gt = 1 - gt
            else:
                gt = (gt == 1).long()
            if p.shape != gt.shape:
                iy = torch.arange(gt.shape[0]) * p.shape[0] // gt.shape[0]
                ix = torch.arange(gt.shape[1]) * p.shape[1] // gt.shape[1]
                p = p[iy][:, ix]
            stats.append(bo.surface_stats(p[None], gt[None], 1, 90.0))
        merged = {k: np.concatenate([s[k] for s in stats]) for k in stats[0]}
        _per, want, want_defined = bo.metrics(merged)
        means, defined = evaluate_surface_distances(Stub(), loader, device=dev, binarize=binarize, percentile=90.0)
        assert defined == want_defined == 2, (binarize, defined)
        for key in ("hd", "hd95", "assd"):
            assert abs(means[key] - want[key]) <= 1e-12 * want[key] and want[key] > 0, (binarize, key, means, want)
