"""The overlap sums, the Tversky / soft Dice loss, the focal loss, their criteria and a planned training step with
``CrossEntropyTverskyLoss`` on the device (csrc/overlap_loss.hip) against the oracle of tests/overlap_loss_oracle.py.

Parity bound of every loss, map and gradient (the rule of tests/test_hip_boundary_loss.py with a floor): the SAME oracle run in
torch float32 on the CPU against its float64 run is the yardstick, computed here per case; the device may be off the float64
value by at most ``max(4 x that, 2^-23 x |float64 value|)`` - the largest magnitude for a gradient or a map.  The floor is one
float32 rounding of the output: where the float32 oracle happens to land within half an ulp (it does at 1x2x1x7), 4 x its error
alone would refuse a correctly rounded result.  The worst ratios are reported with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_loss_oracle as oo  # noqa: E402

pytestmark = pytest.mark.gpu

IGNORE = oo.IGNORE
FLOOR = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(logits, labels) of one shape - made once, shared, never written."""
    B, C, H, W = oo.SHAPES[case]
    return oo.make_logits(B, C, H, W, 300 + case), oo.make_labels(B, C, H, W, 400 + case)


def shape_name(case):
    return "x".join(str(v) for v in oo.SHAPES[case])


def bound(yard, ref):
    return max(4.0 * yard, FLOOR * float(ref.abs().max()))


def check(what, got, want64, want32):
    """The error of ``got`` against ``want64``, the yardstick and the bound; returns error / bound after asserting."""
    err = (got.double() - want64).abs().max().item()
    yard = (want32.double() - want64).abs().max().item()
    b = bound(yard, want64)
    print(f"{what}: device error {err:.3e}, float32 oracle {yard:.3e}, bound {b:.3e}")
    assert torch.isfinite(got).all(), what
    assert err <= b, (what, err, yard, b)
    return err / b if b > 0 else 0.0


def device_tversky(dev, logits, labels, fn=None, **kw):
    from weaklysuperviseddl_amd import ops
    z = logits.to(dev).requires_grad_()
    loss = (fn or ops.tversky_loss)(z, labels.to(dev), **kw)
    loss.backward()
    return loss.detach().cpu(), z.grad.cpu()


def device_focal(dev, logits, labels, **kw):
    from weaklysuperviseddl_amd import ops
    z = logits.to(dev).requires_grad_()
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    loss = ops.focal_loss(z, labels.to(dev), **kw)
    loss.sum().backward() if loss.dim() else loss.backward()
    return loss.detach().cpu(), z.grad.cpu()


def class_lists(C):
    return [cl for cl in oo.CLASS_LISTS if cl is None or max(cl) < C]


# ------------------------------------------------------------------------------------------------------ 1. overlap sums
@pytest.mark.parametrize("case", range(len(oo.SHAPES)))
def test_overlap_sums_against_float64(dev, case):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    logits, labels = inputs(case)
    C = oo.SHAPES[case][1]
    worst = 0.0
    for per_image in (False, True):
        for classes in class_lists(C):
            want = oo.overlap_sums(logits, labels, classes, IGNORE, per_image)
            w32 = oo.overlap_sums(logits, labels, classes, IGNORE, per_image, torch.float32)
            got = ops.overlap_sums(logits.to(dev), labels.to(dev), classes=classes, ignore_index=IGNORE, per_image=per_image)
            assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
            got = got.cpu()
            assert torch.equal(got[..., 2], want[..., 2]), (per_image, classes)          # Y: exact
            for q, name in ((0, "I"), (1, "P")):
                worst = max(worst, check(f"overlap sums {shape_name(case)} per_image={per_image} classes={classes} {name}",
                                         got[..., q], want[..., q], w32[..., q]))
            assert (got[..., 0] <= got[..., 1]).all() and (got[..., 0] <= got[..., 2]).all()
            again = ops.overlap_sums(logits.to(dev), labels.to(dev), classes=classes, ignore_index=IGNORE, per_image=per_image)
            assert torch.equal(again.cpu(), got)                                          # bitwise reproducible
    report_line(f"overlap sums {shape_name(case)}: worst |device - float64| / bound {worst:.3f}")


def test_overlap_sums_reuse_the_callers_buffer(dev):
    from weaklysuperviseddl_amd import ops
    logits, labels = inputs(3)
    bufs = {}
    first = ops.overlap_sums(logits.to(dev), labels.to(dev), ignore_index=IGNORE, per_image=True, out=bufs)
    assert first is bufs["sums"] and tuple(first.shape) == (3, 3, 3)
    ptr, keep = first.data_ptr(), first.clone()
    again = ops.overlap_sums(logits.to(dev), labels.to(dev), ignore_index=IGNORE, per_image=True, out=bufs)
    assert again.data_ptr() == ptr and torch.equal(again, keep)
    with pytest.raises(ops.WsdlError):
        ops.overlap_sums(logits.to(dev), labels.to(dev)[:, :5])


# ------------------------------------------------------------------------------------------------------ 2. Tversky
@pytest.mark.parametrize("case", range(len(oo.SHAPES)))
def test_tversky_loss_and_gradient_against_float64(dev, case):
    from conftest import report_line
    logits, labels = inputs(case)
    B, C, H, W = oo.SHAPES[case]
    worst_l = worst_g = 0.0
    for alpha, beta, gamma in oo.TVERSKY:
        for per_image in (False, True):
            for classes in class_lists(C):
                kw = dict(alpha=alpha, beta=beta, gamma=gamma, smooth=1.0, classes=classes, per_image=per_image, ignore_index=IGNORE)
                l64, g64 = oo.tversky(logits, labels, **kw)
                l32, g32 = oo.tversky(logits, labels, dtype=torch.float32, **kw)
                loss, grad = device_tversky(dev, logits, labels, **kw)
                assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32 and tuple(grad.shape) == (B, C, H, W)
                tag = f"tversky {shape_name(case)} ({alpha},{beta},{gamma}) per_image={per_image} classes={classes}"
                worst_l = max(worst_l, check(tag + " loss", loss, l64, l32))
                worst_g = max(worst_g, check(tag + " gradient", grad, g64, g32))
                assert (grad.permute(0, 2, 3, 1)[labels == IGNORE] == 0).all()      # invalid pixels: exactly 0
                # sum over C of s_j (g_j - dot): C float32 roundings of at most the largest gradient
                assert grad.double().sum(dim=1).abs().max().item() <= C * 2.0 ** -24 * max(grad.abs().max().item(), 1e-30)
                l2, g2 = device_tversky(dev, logits, labels, **kw)
                assert torch.equal(l2, loss) and torch.equal(g2, grad)              # bitwise reproducible
    report_line(f"tversky {shape_name(case)}: worst |device - float64| / bound: loss {worst_l:.3f}, gradient {worst_g:.3f}")


def test_present_only_drops_the_class_an_image_lacks(dev):
    from conftest import report_line
    logits, labels = inputs(3)                                           # 3x3x37x53
    labels = labels.clone()
    labels[1][labels[1] == 2] = 0                                        # image 1 has no pixel of class 2
    worst = 0.0
    for per_image in (True, False):
        for classes in (None, (2, 0)):
            kw = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, classes=classes, per_image=per_image, ignore_index=IGNORE)
            l64, g64 = oo.tversky(logits, labels, present_only=True, **kw)
            l32, g32 = oo.tversky(logits, labels, present_only=True, dtype=torch.float32, **kw)
            loss, grad = device_tversky(dev, logits, labels, present_only=True, **kw)
            worst = max(worst, check(f"present_only per_image={per_image} classes={classes} loss", loss, l64, l32),
                        check(f"present_only per_image={per_image} classes={classes} gradient", grad, g64, g32))
            full, gfull = device_tversky(dev, logits, labels, present_only=False, **kw)
            # the term is dropped only where a segment lacks the class: per image, not in the batch as a whole
            assert (float(full) != float(loss)) == per_image
            if per_image:
                assert not torch.equal(gfull[1], grad[1])
    report_line(f"tversky present_only 3x3x37x53: worst |device - float64| / bound {worst:.3f}")


def test_tversky_edge_cases(dev):
    from weaklysuperviseddl_amd import ops
    logits, labels = inputs(3)
    # no valid pixel: loss 0 and a zero gradient, not NaN
    void = torch.full_like(labels, IGNORE)
    for per_image in (False, True):
        loss, grad = device_tversky(dev, logits, void, per_image=per_image, ignore_index=IGNORE)
        assert float(loss) == 0.0 and not grad.any() and torch.isfinite(grad).all()
    # smooth = 0 with a class that is absent from the batch: finite, and the oracle's numbers
    absent = torch.where(labels == 2, torch.zeros_like(labels), labels)
    kw = dict(alpha=0.5, beta=0.5, gamma=1.0, smooth=0.0, per_image=True, ignore_index=IGNORE)
    loss, grad = device_tversky(dev, logits, absent, **kw)
    l64, g64 = oo.tversky(logits, absent, **kw)
    l32, g32 = oo.tversky(logits, absent, dtype=torch.float32, **kw)
    check("smooth = 0, absent class: loss", loss, l64, l32)
    check("smooth = 0, absent class: gradient", grad, g64, g32)
    # a device scale of 0 gives exactly 0; a power of two is exact
    scale = torch.zeros(1, device=dev)
    l0, g0 = device_tversky(dev, logits, labels, ignore_index=IGNORE, scale=scale)
    assert float(l0) == 0.0 and not g0.any()
    l1, g1 = device_tversky(dev, logits, labels, ignore_index=IGNORE)
    scale.fill_(2.0)
    l2, g2 = device_tversky(dev, logits, labels, ignore_index=IGNORE, scale=scale)
    assert torch.equal(l2, l1 * 2) and torch.equal(g2, g1 * 2) and g1.abs().sum() > 0
    # dice_loss is the tversky_loss call it is defined as, bit for bit
    for smooth in (1.0, 0.0, 2.5):
        ld, gd = device_tversky(dev, logits, labels, fn=ops.dice_loss, smooth=smooth, classes=(1,), per_image=True, ignore_index=IGNORE)
        lt, gt = device_tversky(dev, logits, labels, alpha=0.5, beta=0.5, gamma=1.0, smooth=smooth / 2, classes=(1,), per_image=True,
                                ignore_index=IGNORE)
        assert torch.equal(ld, lt) and torch.equal(gd, gt)
    with pytest.raises(ops.WsdlError):
        ops.tversky_loss(logits.to(dev), labels.to(dev), scale=torch.ones(2, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.tversky_loss(logits.to(dev), labels.to(dev)[:, :5])
    with pytest.raises(ValueError):
        ops.tversky_loss(logits.to(dev), labels.to(dev), classes=(3,))


@pytest.mark.parametrize("C", (2, 3, 5))
def test_a_view_at_an_odd_storage_offset_takes_the_scalar_path(dev, C):
    """(2,C,8,8): H W is a multiple of 4, so the aligned call runs four pixels per lane; a contiguous view that starts one
    element into its storage is 4 (logits) / 8 (labels) bytes off a 16-byte boundary and runs one pixel per lane.  The two paths
    add in another order, so the results agree within the bound, not bit for bit."""
    from weaklysuperviseddl_amd import ops
    B, H, W = 2, 8, 8
    logits, labels = oo.make_logits(B, C, H, W, 77), oo.make_labels(B, C, H, W, 78)
    n = logits.numel()
    z_off = torch.empty(n + 1, device=dev)[1:].view(B, C, H, W).copy_(logits)
    y_off = torch.empty(labels.numel() + 1, dtype=torch.int64, device=dev)[1:].view(B, H, W).copy_(labels)
    assert z_off.is_contiguous() and z_off.data_ptr() % 16 == 4 and y_off.data_ptr() % 16 == 8
    for kw in (dict(), dict(per_image=True, classes=(1,), alpha=0.3, beta=0.7, gamma=0.75)):
        l64, g64 = oo.tversky(logits, labels, ignore_index=IGNORE, **kw)
        l32, g32 = oo.tversky(logits, labels, ignore_index=IGNORE, dtype=torch.float32, **kw)
        la, ga = device_tversky(dev, logits, labels, ignore_index=IGNORE, **kw)
        for z, y in ((z_off, labels.to(dev)), (logits.to(dev), y_off)):
            z = z.detach().requires_grad_()
            loss = ops.tversky_loss(z, y, ignore_index=IGNORE, **kw)
            loss.backward()
            check(f"odd offset C={C} loss", loss.detach().cpu(), l64, l32)
            check(f"odd offset C={C} gradient", z.grad.cpu(), g64, g32)
            assert abs(float(loss.detach()) - float(la)) <= bound(abs(float(l32) - float(l64)), l64)
            assert (z.grad.cpu() - ga).abs().max().item() <= bound((g32.double() - g64).abs().max().item(), g64)
    f64, fg64 = oo.focal(logits, labels, 2.0, ignore_index=IGNORE)
    f32, fg32 = oo.focal(logits, labels, 2.0, ignore_index=IGNORE, dtype=torch.float32)
    z = z_off.detach().requires_grad_()
    loss = ops.focal_loss(z, y_off, ignore_index=IGNORE)
    loss.backward()
    check(f"odd offset C={C} focal loss", loss.detach().cpu(), f64, f32)
    check(f"odd offset C={C} focal gradient", z.grad.cpu(), fg64, fg32)


# ------------------------------------------------------------------------------------------------------ 3. focal
def ulps(a, b):
    a, b = a.double(), b.double()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    return ((a - b).abs() / torch.exp2(torch.floor(torch.log2(mag)) - 23)).max().item()


@pytest.mark.parametrize("case", range(len(oo.SHAPES)))
def test_focal_loss_and_gradient_against_float64(dev, case):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    logits, labels = inputs(case)
    B, C, H, W = oo.SHAPES[case]
    g = torch.Generator().manual_seed(500 + case)
    cw = torch.rand(C, generator=g) + 0.25
    pw = torch.rand(B, H, W, generator=g)
    if H * W > 1:
        pw[0, 0, 0] = 0.0                                                # a pixel of weight 0 is an ignored pixel
    worst_l = worst_g = 0.0
    for gamma in (0.0, 0.5, 2.0):
        for wname, kw in (("none", {}), ("class", dict(weight=cw)), ("pixel", dict(pixel_weight=pw))):
            for reduction in ("mean", "sum", "none"):
                okw = dict(gamma=gamma, ignore_index=IGNORE, reduction=reduction, **kw)
                l64, g64 = oo.focal(logits, labels, **okw)
                l32, g32 = oo.focal(logits, labels, dtype=torch.float32, **okw)
                loss, grad = device_focal(dev, logits, labels, **okw)
                assert loss.dtype == torch.float32 and tuple(loss.shape) == ((B, H, W) if reduction == "none" else ())
                tag = f"focal {shape_name(case)} gamma={gamma} weights={wname} {reduction}"
                worst_l = max(worst_l, check(tag + " loss", loss, l64, l32))
                worst_g = max(worst_g, check(tag + " gradient", grad, g64, g32))
                assert (grad.permute(0, 2, 3, 1)[labels == IGNORE] == 0).all()
                if wname == "pixel" and H * W > 1:
                    assert not grad[0, :, 0, 0].any() and (reduction != "none" or float(loss[0, 0, 0]) == 0.0)
    # gamma = 0 is the cross entropy: the distance to the library's own kernel, recorded (that one sums in float32)
    z1, z2 = logits.to(dev).requires_grad_(), logits.to(dev).requires_grad_()
    lf = ops.focal_loss(z1, labels.to(dev), gamma=0.0, ignore_index=IGNORE)
    lc = ops.cross_entropy(z2, labels.to(dev), IGNORE)
    lf.backward()
    lc.backward()
    d_l, d_g = ulps(lf.detach().cpu(), lc.detach().cpu()), (z1.grad - z2.grad).abs().max().item()
    print(f"focal {shape_name(case)} gamma=0 against ops.cross_entropy: loss {d_l:.2f} ulp, gradient max |difference| {d_g:.3e}")
    report_line(f"focal {shape_name(case)}: worst |device - float64| / bound: loss {worst_l:.3f}, gradient {worst_g:.3f}; "
                f"gamma=0 against ops.cross_entropy: loss {d_l:.2f} ulp, gradient {d_g:.2e}")


def test_focal_stays_finite_at_logit_gaps_of_forty_and_poisons_bad_labels(dev):
    """Gaps of +-40: where the label holds the +40, 1 - s_y by subtraction rounds to 0 (q is 8.5e-18); where it holds the -40,
    s_y is about 4e-18.  The last pixel has no gap."""
    z = torch.zeros(1, 3, 1, 4)
    z[0, 0] = torch.tensor([40.0, -40.0, 40.0, 0.0])
    labels = torch.tensor([[[0, 0, 1, 2]]])
    for gamma in (0.0, 0.5, 2.0):
        for reduction in ("none", "mean", "sum"):
            l64, g64 = oo.focal(z, labels, gamma, reduction=reduction)
            l32, g32 = oo.focal(z, labels, gamma, reduction=reduction, dtype=torch.float32)
            loss, grad = device_focal(dev, z, labels, gamma=gamma, reduction=reduction)
            check(f"focal +-40 gamma={gamma} {reduction} loss", loss, l64, l32)
            check(f"focal +-40 gamma={gamma} {reduction} gradient", grad, g64, g32)
            if reduction == "none":
                assert float(loss[0, 0, 0]) > 0 or gamma > 0            # 8.5e-18 is a float32; its square is not
                assert abs(float(loss[0, 0, 1]) - 40.693147) < 1e-4
    bad = torch.tensor([[[0, 7, 1, IGNORE]]])
    loss, grad = device_focal(dev, z, bad, gamma=2.0, ignore_index=IGNORE, reduction="none")
    assert torch.isnan(loss[0, 0, 1]) and torch.isfinite(loss[0, 0, [0, 2, 3]]).all() and float(loss[0, 0, 3]) == 0.0
    assert not grad[0, :, 0, 3].any()
    for reduction in ("mean", "sum"):
        assert torch.isnan(device_focal(dev, z, bad, gamma=2.0, ignore_index=IGNORE, reduction=reduction)[0])
    assert torch.isnan(device_focal(dev, z, bad, gamma=2.0, ignore_index=IGNORE, reduction="mean",
                                    weight=torch.tensor([1.0, 2.0, 3.0]))[0])


# ------------------------------------------------------------------------------------------------------ 4. modules
def test_modules_equal_their_ops_bit_for_bit(dev):
    from weaklysuperviseddl_amd import ops, nn as wnn
    logits, labels = inputs(3)
    logits, labels = logits.to(dev), labels.to(dev)
    cw = torch.tensor([0.7, 1.9, 0.4])
    pw = torch.rand(3, 37, 53, generator=torch.Generator().manual_seed(1)).to(dev)
    tv = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=0.5, classes=(2, 0), per_image=True, present_only=True, ignore_index=IGNORE)
    pairs = (
        (wnn.TverskyLoss(**tv), lambda z: ops.tversky_loss(z, labels, **tv)),
        (wnn.TverskyLoss(ignore_index=IGNORE), lambda z: ops.tversky_loss(z, labels, ignore_index=IGNORE)),
        (wnn.DiceLoss(smooth=2.0, classes=(1,), ignore_index=IGNORE), lambda z: ops.dice_loss(z, labels, smooth=2.0, classes=(1,), ignore_index=IGNORE)),
        (wnn.FocalLoss(gamma=1.5, weight=cw, ignore_index=IGNORE, reduction="sum").to(dev).set_pixel_weight(pw),
         lambda z: ops.focal_loss(z, labels, gamma=1.5, weight=cw.to(dev), ignore_index=IGNORE, reduction="sum", pixel_weight=pw)),
        (wnn.FocalLoss(ignore_index=IGNORE), lambda z: ops.focal_loss(z, labels, ignore_index=IGNORE)),
    )
    for crit, fn in pairs:
        za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
        la, lb = crit(za, labels), fn(zb)
        la.backward()
        lb.backward()
        assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0, crit
    focal = pairs[3][0]
    ptr = focal.pixel_weight_ptr
    focal.set_pixel_weight(pw * 0.5)
    assert focal.pixel_weight_ptr == ptr == focal.pixel_weight.data_ptr() and focal.pixel_weight_shape == "3x37x53"


@pytest.mark.parametrize("weighted", (False, True))
def test_lam_zero_is_the_cross_entropy_bit_for_bit(dev, weighted):
    from weaklysuperviseddl_amd import nn as wnn
    logits, labels = inputs(5)                                           # 2x2x96x130
    kw = dict(ignore_index=IGNORE)
    if weighted:
        kw.update(weight=torch.tensor([0.7, 1.9]), label_smoothing=0.1)
    logits, labels = logits.to(dev), labels.to(dev)
    crit = wnn.CrossEntropyTverskyLoss(lam=0.0, alpha=0.3, beta=0.7, **kw).to(dev)
    ref = wnn.CrossEntropyLoss(**kw).to(dev)
    za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    la, lb = crit(za, labels), ref(zb, labels)
    la.backward()
    lb.backward()
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0
    # with lam > 0 it is the sum of the two terms
    crit.set_lam(0.25)
    zc, zd = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    lc = crit(zc, labels)
    tl = wnn.TverskyLoss(alpha=0.3, beta=0.7, ignore_index=IGNORE)(zd, labels)
    lc, lb, tl = lc.item(), lb.item(), tl.item()
    assert lc != lb and abs(lc - (lb + 0.25 * tl)) <= 2.0 ** -22 * (abs(lb) + abs(tl))


# ------------------------------------------------------------------------------------------------------ 5. launch plan
def test_planned_step_replays_through_set_lam_and_records_anew_for_another_alpha(dev):
    """The pattern of the boundary-loss plan test: ten steps on the reference's model at 4 x 64 x 64, two batches with different
    masks in turn: eager, eager, record (+ verification on a probe batch), replay; then ``set_lam`` - the SAME plan replays
    three more times; then ``alpha`` changes: eager (a key seen once), record, replay.  Every loss and the final state equal the
    eager run's (``WSDL_PLAN_STEP=0``) bit for bit; a run that keeps the old lam - what a plan with a frozen lam would compute -
    has another loss at step 5."""
    from weaklysuperviseddl_amd import plan, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(4, 3, 64, 64, generator=g).to(dev), torch.randint(0, 2, (4, 64, 64), generator=g).to(dev)) for _ in range(2)]
    assert not torch.equal(batches[0][1], batches[1][1])

    def run(planned, schedule):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = build_segmentation_model().to(dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = wnn.CrossEntropyTverskyLoss(lam=schedule[0][0], alpha=schedule[0][1], beta=0.7, classes=(1,)).to(dev)
            torch.manual_seed(1234)
            losses, plans = [], []
            st = None
            for i, (lam, alpha) in enumerate(schedule):
                crit.set_lam(lam)
                crit.tversky.alpha = alpha
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
                st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
                plans.append(None if st is None else (id(st), st.records, st.replays))
            torch.cuda.synchronize()
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st, plans
        finally:
            plan.PLAN_STEP[0] = old

    schedule = [(0.5, 0.3)] * 4 + [(2.0, 0.3)] * 3 + [(2.0, 0.6)] * 3
    l0, s0, _, _ = run(False, schedule)
    l1, s1, st, plans = run(True, schedule)
    stale, _, _, _ = run(False, [(0.5, 0.3)] * 5)
    print(f"planned CE + Tversky step: losses {l1}, records {st.records}, replays {st.replays}; step 5 with the old lam {stale[4]}")
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert plans[3][1:] == (1, 1) and plans[6][1:] == (1, 4), plans      # after set_lam: the same plan, no new recording
    assert len({p[0] for p in plans if p is not None}) == 1
    assert st.records == 2 and st.replays == 5, (st.records, st.replays)  # another alpha: a new plan
    assert l0 == l1 and all(v == v for v in l0), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert stale[:4] == l0[:4] and stale[4] != l0[4]
