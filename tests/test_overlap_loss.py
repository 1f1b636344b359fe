"""The oracle of tests/overlap_loss_oracle.py against independent formulations on the CPU - torch autograd of the direct
definitions (one-hot ``einsum``, ``sum``, ``mean``) in float64, the closed-form Tversky gradient, the textbook Dice quotient,
``torch.nn.functional.cross_entropy`` for the focal loss at gamma = 0 and autograd of ``(1 - s_y)^gamma (-log s_y)`` - the
host arithmetic of ``ops.dice_from_counts``, every option check that needs no device, and the argument checks of the C ABI
(they return before any launch, so the built library is enough)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_loss_oracle as oo  # noqa: E402

IGNORE = oo.IGNORE


def direct_tversky(z, labels, alpha, beta, gamma, smooth, classes, per_image, present_only, ignore):
    """The definition, term by term, for autograd: z float64 with requires_grad."""
    s = torch.softmax(z, dim=1)
    valid = (labels != ignore).double()
    terms = []
    segs = [slice(b, b + 1) for b in range(z.shape[0])] if per_image else [slice(None)]
    for sl in segs:
        for c in classes:
            y = ((labels[sl] == c).double() * valid[sl])
            I = torch.einsum("bhw,bhw->", s[sl, c], y)
            P = (s[sl, c] * valid[sl]).sum()
            Y = y.sum()
            if present_only and Y.item() == 0:
                continue
            N = I + smooth
            D = I + alpha * (P - I) + beta * (Y - I) + smooth
            if D.item() == 0 or (1 - N / D).item() <= 0:
                terms.append(0.0 * I)
            else:
                terms.append((1 - N / D) ** gamma)
    if not terms:
        return 0.0 * s.sum()
    return torch.stack(terms).mean()


@pytest.mark.parametrize("abg", oo.TVERSKY)
@pytest.mark.parametrize("per_image", (False, True))
@pytest.mark.parametrize("C,classes", ((2, None), (3, (1,)), (3, (2, 0)), (21, (2, 0)), (5, None)))
def test_tversky_equals_autograd_of_the_definition(abg, per_image, C, classes):
    alpha, beta, gamma = abg
    B, H, W = 3, 9, 11
    labels = oo.make_labels(B, C, H, W, 11)
    z = oo.make_logits(B, C, H, W, 3).double().requires_grad_()
    cl = tuple(range(C)) if classes is None else classes
    for present_only, smooth in ((False, 1.0), (True, 0.0)):
        ref = direct_tversky(z, labels, alpha, beta, gamma, smooth, cl, per_image, present_only, IGNORE)
        z.grad = None
        ref.backward()
        got, grad = oo.tversky(z.detach(), labels, alpha, beta, gamma, smooth, classes, per_image, present_only, IGNORE)
        assert abs(float(got) - ref.item()) <= 1e-15, (float(got), ref.item())
        assert (grad - z.grad).abs().max().item() <= 1e-16, (grad - z.grad).abs().max().item()
        assert (grad.permute(0, 2, 3, 1)[labels == IGNORE] == 0).all() and (labels == IGNORE).any()
        # softmax gradients sum to 0 over C: sum_j s_j (g_j - dot) with dot = sum_c s_c g_c - C products and C additions each
        # in the dot product and in the sum, every one rounded to 2^-53 of at most max|g| = max(|a| + |b|)
        _, a, b = oo.tversky_from_sums(oo.overlap_sums(z.detach(), labels, cl, IGNORE, per_image), alpha, beta, gamma, smooth,
                                       present_only, 1.0)
        assert grad.sum(dim=1).abs().max().item() <= (2 * C + 2) * 2.0 ** -53 * (a.abs() + b.abs()).max().item()
        ls, gs = oo.tversky(z.detach(), labels, alpha, beta, gamma, smooth, classes, per_image, present_only, IGNORE, scale=0.37)
        assert abs(float(ls) - 0.37 * float(got)) <= 1e-16 and (gs - 0.37 * grad).abs().max().item() <= 1e-17
    l32, g32 = oo.tversky(z.detach().float(), labels, alpha, beta, gamma, 1.0, classes, per_image, False, IGNORE, dtype=torch.float32)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32 and abs(float(l32) - float(got)) < 1.0


def test_closed_form_coefficients_are_the_derivative_of_the_term():
    """a y + b against autograd of the loss with respect to the PROBABILITIES (the sums are linear in them)."""
    sums = torch.tensor([[[3.0, 7.5, 6.0], [0.0, 2.0, 0.0]], [[1.25, 1.5, 9.0], [4.0, 4.0, 4.0]]], dtype=torch.float64)
    for alpha, beta, gamma in oo.TVERSKY:
        for present_only in (False, True):
            x = sums.clone().requires_grad_()
            loss, a, b = oo.tversky_from_sums(x, alpha, beta, gamma, 0.5, present_only, 1.0)
            loss.backward()
            # d loss / d s at a pixel with y = 1 moves I and P together, with y = 0 only P
            # (a handful of double roundings, each 2^-53 of at most the largest coefficient; observed ~ 1e-17)
            tol = 8 * 2.0 ** -53 * (a.abs() + b.abs()).max().item()
            assert (x.grad[..., 1] - b).abs().max().item() <= tol
            assert (x.grad[..., 0] + x.grad[..., 1] - (a + b)).abs().max().item() <= tol
            assert (a[0, 1] == 0 and b[0, 1] == 0) == present_only      # the absent class is dropped only with present_only
    # a perfect prediction: 1 - T == 0, the term and both coefficients are exactly 0
    loss, a, b = oo.tversky_from_sums(torch.tensor([[[4.0, 4.0, 4.0]]], dtype=torch.float64), 0.3, 0.7, 0.75, 1.0, False, 1.0)
    assert float(loss) == 0 and not a.any() and not b.any()


@pytest.mark.parametrize("per_image", (False, True))
def test_dice_equals_the_textbook_quotient(per_image):
    B, C, H, W = 2, 3, 5, 7
    labels = oo.make_labels(B, C, H, W, 5)
    z = oo.make_logits(B, C, H, W, 6).double()
    for smooth in (1.0, 0.0, 2.5):
        sums = oo.overlap_sums(z, labels, None, IGNORE, per_image)
        I, P, Y = sums[..., 0], sums[..., 1], sums[..., 2]
        want = (1 - (2 * I + smooth) / (P + Y + smooth)).mean()
        got, _ = oo.dice(z, labels, smooth, per_image=per_image, ignore_index=IGNORE)
        assert abs(float(got) - float(want)) <= 1e-15
    assert torch.equal(sums[..., 2], torch.stack([((labels == c) & (labels != IGNORE)).flatten(1).sum(1).double() for c in range(C)], 1)
                       if per_image else torch.stack([((labels == c)).sum().double() for c in range(C)])[None])


def test_edge_rules_of_the_tversky_oracle():
    z = oo.make_logits(2, 3, 5, 7, 1).double()
    void = torch.full((2, 5, 7), IGNORE)
    loss, grad = oo.tversky(z, void, ignore_index=IGNORE)
    assert float(loss) == 0 and not grad.any()                          # no valid pixel: 0, not NaN
    labels = torch.zeros(2, 5, 7, dtype=torch.int64)
    labels[0, :2] = 1                                                   # class 2 nowhere, class 1 only in image 0
    loss, grad = oo.tversky(z, labels, 0.5, 0.5, 1.0, 0.0, per_image=True)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()          # smooth = 0 with an absent class
    full, _ = oo.tversky(z, labels, per_image=True)
    present, _ = oo.tversky(z, labels, per_image=True, present_only=True)
    sums = oo.overlap_sums(z, labels, per_image=True)
    kept = sums[..., 2] != 0
    assert int(kept.sum()) == 3 and float(full) != float(present)
    _, a, b = oo.tversky_from_sums(sums, 0.5, 0.5, 1.0, 1.0, True, 1.0)
    assert not a[~kept].any() and not b[~kept].any() and a[kept].all()
    zero, gz = oo.tversky(z, labels, scale=0.0)
    assert float(zero) == 0 and not gz.any()


# ------------------------------------------------------------------------------------------------------------ focal
def focal_inputs(C=4, seed=2):
    B, H, W = 2, 6, 7
    labels = oo.make_labels(B, C, H, W, seed)
    z = oo.make_logits(B, C, H, W, seed + 1).double()
    g = torch.Generator().manual_seed(seed + 2)
    weight = torch.rand(C, generator=g).double() + 0.25
    pw = torch.rand(B, H, W, generator=g).double()
    pw[0, 3, :3] = 0.0
    return z, labels, weight, pw


@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_focal_at_gamma_zero_is_the_weighted_cross_entropy(reduction):
    z, labels, weight, _ = focal_inputs()
    for w in (None, weight):
        x = z.clone().requires_grad_()
        ref = F.cross_entropy(x, labels, weight=w, ignore_index=IGNORE, reduction=reduction)
        ref.sum().backward()
        got, grad = oo.focal(z, labels, 0.0, w, IGNORE, reduction)
        assert (got - ref.detach()).abs().max().item() <= 1e-14 * max(1.0, ref.detach().abs().max().item())
        assert (grad - x.grad).abs().max().item() <= 1e-15


@pytest.mark.parametrize("gamma", (0.5, 1.0, 2.0, 5.0))
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_focal_equals_autograd_of_the_definition(gamma, reduction):
    z, labels, weight, pw = focal_inputs()
    x = z.clone().requires_grad_()
    logp = torch.log_softmax(x, dim=1)
    valid = (labels != IGNORE) & (pw != 0)
    lab = torch.where(labels == IGNORE, torch.zeros_like(labels), labels)
    lsy = logp.gather(1, lab[:, None])[:, 0]
    wy = pw * weight[lab] * valid.double()
    l = wy * (1 - lsy.exp()) ** gamma * (-lsy)
    ref = {"none": l, "sum": l.sum(), "mean": l.sum() / wy.sum()}[reduction]
    ref.sum().backward()
    got, grad = oo.focal(z, labels, gamma, weight, IGNORE, reduction, pw)
    assert (got - ref.detach()).abs().max().item() <= 1e-14
    assert (grad - x.grad).abs().max().item() <= 1e-14
    assert (grad.permute(0, 2, 3, 1)[~valid] == 0).all() and (~valid).sum() > 3
    assert grad.sum(dim=1).abs().max().item() <= 1e-15


def test_focal_edge_rules():
    # logit gaps of +-40: 1 - s_y by subtraction would be 0 / s_y ~ 4e-18; everything stays finite and non-trivial
    z = torch.zeros(1, 3, 1, 4)
    z[0, 0] = torch.tensor([40.0, -40.0, 40.0, 0.0])
    labels = torch.tensor([[[0, 0, 1, 2]]])
    for gamma in (0.0, 0.5, 2.0):
        for dtype in (torch.float64, torch.float32):
            l, g = oo.focal(z, labels, gamma, reduction="none", dtype=dtype)
            assert torch.isfinite(l).all() and torch.isfinite(g).all(), (gamma, dtype)
        l, g = oo.focal(z, labels, gamma, reduction="none")
        q = 2 * np.exp(-40.0) / (1 + 2 * np.exp(-40.0))
        assert abs(float(l[0, 0, 0]) - q ** gamma * np.log1p(2 * np.exp(-40.0))) <= 1e-30 and float(l[0, 0, 0]) > 0
        assert abs(float(l[0, 0, 1]) - (40.0 + np.log(2.0))) <= 1e-12      # s_y = 1 / (1 + 2 e^40): q^gamma is 1 to 1e-17
    # a label that is no class and not ignore_index: NaN there and only there
    bad = torch.tensor([[[0, 7, 1, IGNORE]]])
    l, g = oo.focal(z, bad, 2.0, ignore_index=IGNORE, reduction="none")
    assert torch.isnan(l[0, 0, 1]) and torch.isfinite(l[0, 0, [0, 2, 3]]).all() and float(l[0, 0, 3]) == 0
    assert torch.isnan(oo.focal(z, bad, 2.0, ignore_index=IGNORE)[0])
    assert torch.isnan(oo.focal(z, torch.full((1, 1, 4), IGNORE), 2.0, ignore_index=IGNORE)[0])      # 0 / 0


# ------------------------------------------------------------------------------------------------------------ host side
def test_dice_from_counts_against_numpy():
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(0)
    inter = rng.integers(0, 50, (4, 3))
    union = inter + rng.integers(0, 50, (4, 3))
    union[1, 2] = inter[1, 2] = 0                                        # an empty class in one image
    counts = np.stack([inter, union], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(union > 0, 2.0 * inter / (inter + union), 1.0)
    assert np.allclose(ops.dice_from_counts(counts), 100 * per.mean(axis=0), rtol=1e-15, atol=0)
    assert np.allclose(ops.dice_from_counts(counts, EMPTY=0.0, ignore=0), 100 * np.where(union > 0, per, 0.0).mean(axis=0)[1:], rtol=1e-15)
    one = ops.dice_from_counts(counts[:1])
    assert one.dtype == np.float64 and np.array_equal(one, 100 * per[0])
    # Dice >= IoU, equal only at 0 and 1
    assert (ops.dice_from_counts(counts) >= ops.iou_from_counts(counts)).all()


def test_option_checks_need_no_device():
    from weaklysuperviseddl_amd import ops, plan, nn as wnn
    z, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    for bad in (-0.1, float("inf"), float("nan"), True, None, "1"):
        for kw in (dict(alpha=bad), dict(beta=bad), dict(smooth=bad), dict(gamma=bad)):
            with pytest.raises(ValueError):
                ops.tversky_loss(z, y, **kw)
            with pytest.raises(ValueError):
                wnn.TverskyLoss(**kw)
            with pytest.raises(ValueError):
                wnn.CrossEntropyTverskyLoss(**kw)
        with pytest.raises(ValueError):
            ops.dice_loss(z, y, smooth=bad)
        with pytest.raises(ValueError):
            wnn.DiceLoss(smooth=bad)
        with pytest.raises(ValueError):
            ops.focal_loss(z, y, gamma=bad)
        with pytest.raises(ValueError):
            wnn.FocalLoss(gamma=bad)
        with pytest.raises(ValueError):
            wnn.CrossEntropyTverskyLoss(lam=bad)
    with pytest.raises(ValueError):
        ops.tversky_loss(z, y, gamma=0.0)                               # Tversky: gamma > 0
    ops.check_focal_options(0.0, "mean")                                # focal: gamma = 0 is the cross entropy
    for bad in ((), (1, 1), (-1,), (1.0,), (True,), 1, tuple(range(33)), "1", (3,)):
        with pytest.raises(ValueError):
            ops.tversky_loss(z, y, classes=bad)
        with pytest.raises(ValueError):
            ops.overlap_sums(z, y, classes=bad)
        if bad != (3,):                                                 # (C is not known before the first call)
            with pytest.raises(ValueError):
                wnn.TverskyLoss(classes=bad)
    with pytest.raises(ValueError):
        ops.tversky_loss(torch.zeros(1, 33, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))      # all of 33 classes
    assert ops.check_overlap_classes(None, 3) == (0, 1, 2) and ops.check_overlap_classes([2, 0], 3) == (2, 0)
    with pytest.raises(ValueError):
        ops.focal_loss(z, y, reduction="batchmean")
    with pytest.raises(ValueError):
        wnn.FocalLoss(weight=torch.zeros(2, 2))
    with pytest.raises(ValueError):
        wnn.CrossEntropyTverskyLoss(label_smoothing=1.5)
    # no CPU fallback
    for call in (lambda: ops.tversky_loss(z, y), lambda: ops.dice_loss(z, y), lambda: ops.focal_loss(z, y),
                 lambda: ops.overlap_sums(z, y), lambda: wnn.DiceLoss()(z, y), lambda: wnn.FocalLoss()(z, y)):
        with pytest.raises(ops.WsdlError):
            call()

    # the plan key: the Tversky options are in it, lam is not (it lives on the device)
    def key(obj):
        def strip(t):
            if isinstance(t, tuple):
                if len(t) == 2 and isinstance(t[0], str) and t[0].endswith("_ptr"):
                    return None
                return tuple(strip(v) for v in t)
            return t
        return strip(plan.host_scalars(obj))

    base = key(wnn.CrossEntropyTverskyLoss())
    assert base == key(wnn.CrossEntropyTverskyLoss(lam=0.5)) and "classes_key" in str(base) and "lam_dev_ptr" not in str(base)
    for kw in (dict(alpha=0.3), dict(beta=0.7), dict(gamma=0.75), dict(smooth=0.0), dict(classes=(1,)), dict(per_image=True),
               dict(present_only=True), dict(ignore_index=255), dict(label_smoothing=0.1)):
        assert key(wnn.CrossEntropyTverskyLoss(**kw)) != base, kw
    assert key(wnn.FocalLoss()) != key(wnn.FocalLoss(gamma=1.0)) and key(wnn.DiceLoss()) != key(wnn.DiceLoss(smooth=2.0))
    assert key(wnn.DiceLoss()) == key(wnn.DiceLoss(smooth=1.0)) and wnn.DiceLoss(smooth=3.0).smooth == 1.5
    crit = wnn.CrossEntropyTverskyLoss(lam=0.25)
    full = plan.host_scalars(crit)
    ptr = crit.lam_dev.data_ptr()
    assert "lam_dev_ptr" in str(full)
    assert crit.set_lam(0.5) is crit and crit.lam_dev.item() == 0.5 and crit.lam_dev.data_ptr() == ptr
    assert plan.host_scalars(crit) == full
    crit.tversky.alpha = 0.3
    assert plan.host_scalars(crit) != full


def test_the_loss_fn_strings_are_not_extended():
    """The new losses are reached through ``criterion=``; ``loss_fn="dice"`` keeps its refusal."""
    from weaklysuperviseddl_amd.TraditionalModel import train_segmentation_model
    with pytest.raises(ValueError, match="lovasz_hinge"):
        train_segmentation_model("dice", "none")


def test_exports_and_signatures():
    import inspect
    from weaklysuperviseddl_amd import ops, _lib, nn as wnn
    for name in ("wsdl_overlap_workspace", "wsdl_overlap_sums", "wsdl_tversky_fwd_bwd", "wsdl_focal_fwd_bwd"):
        assert name in _lib.SIGNATURES
    kwonly = lambda f: [p for p, v in inspect.signature(f).parameters.items() if v.kind is v.KEYWORD_ONLY]      # noqa: E731
    assert kwonly(ops.tversky_loss) == ["alpha", "beta", "gamma", "smooth", "classes", "per_image", "present_only", "ignore_index", "scale"]
    assert kwonly(ops.overlap_sums) == ["classes", "ignore_index", "per_image", "out"]
    assert kwonly(ops.focal_loss) == ["gamma", "weight", "ignore_index", "reduction", "pixel_weight"]
    assert inspect.signature(ops.focal_loss).parameters["gamma"].default == 2.0
    assert list(inspect.signature(wnn.CrossEntropyTverskyLoss.__init__).parameters)[1:] == [
        "lam", "alpha", "beta", "gamma", "smooth", "classes", "per_image", "present_only", "weight", "ignore_index", "label_smoothing"]
    lib = _lib.lib()
    assert lib.wsdl_overlap_workspace(1, 1) > 0 and lib.wsdl_overlap_workspace(16, 32) > lib.wsdl_overlap_workspace(16, 2)
    assert lib.wsdl_overlap_workspace(0, 1) == 0 and lib.wsdl_overlap_workspace(1, 33) == 0 and lib.wsdl_overlap_workspace(1, 0) == 0


def test_abi_refuses_bad_arguments_before_any_launch():
    """Every check is host-side and comes before the first launch: the pointers are never read (small integers stand in for
    device addresses)."""
    from weaklysuperviseddl_amd import _lib
    lib = _lib.lib()
    p, big = 4096, 1 << 26
    cls = (C.c_int * 2)(0, 1)

    def tv(logits=p, labels=p, cl=cls, K=2, loss=p, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, per_image=0, B=1, Cc=2, H=4,
           W=4, ws=p, nbytes=big):
        return lib.wsdl_tversky_fwd_bwd(logits, labels, cl, K, loss, None, None, None, alpha, beta, gamma, smooth, per_image, 0, B,
                                        Cc, H, W, -100, ws, nbytes, None)

    bad = [dict(logits=None), dict(labels=None), dict(cl=None), dict(loss=None), dict(ws=None), dict(K=0), dict(K=33), dict(B=0),
           dict(Cc=0), dict(H=0), dict(W=-1), dict(cl=(C.c_int * 2)(1, 1)), dict(cl=(C.c_int * 2)(0, 2)), dict(cl=(C.c_int * 2)(-1, 0)),
           dict(alpha=-0.5), dict(beta=-1e-9), dict(smooth=-1.0), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")),
           dict(alpha=float("inf")), dict(per_image=1, B=65536)]
    einval = tv(logits=None)
    assert einval != 0 and b"null pointer" in lib.wsdl_last_error()
    for kw in bad:
        assert tv(**kw) == einval, kw
        assert lib.wsdl_last_error(), kw
    assert b"listed twice" in (tv(cl=(C.c_int * 2)(1, 1)), lib.wsdl_last_error())[1]
    assert b"outside" in (tv(cl=(C.c_int * 2)(0, 2)), lib.wsdl_last_error())[1]
    small = tv(nbytes=8)
    assert small not in (0, einval) and b"workspace" in lib.wsdl_last_error()

    def sums(logits=p, labels=p, cl=cls, K=2, out=p, B=1, Cc=2, H=4, W=4, ws=p, nbytes=big):
        return lib.wsdl_overlap_sums(logits, labels, cl, K, out, B, Cc, H, W, 0, -100, ws, nbytes, None)

    for kw in (dict(logits=None), dict(labels=None), dict(cl=None), dict(out=None), dict(ws=None), dict(K=0), dict(K=3, cl=(C.c_int * 3)(0, 1, 2)),
               dict(B=0), dict(cl=(C.c_int * 2)(0, 0))):
        assert sums(**kw) == einval, kw
    assert sums(nbytes=8) == small

    def focal(logits=p, labels=p, loss=p, dl=None, inv=None, B=1, Cc=2, H=4, W=4, gamma=2.0, red=0, ws=p, nbytes=big):
        return lib.wsdl_focal_fwd_bwd(logits, labels, loss, dl, inv, B, Cc, H, W, gamma, -100, None, None, red, ws, nbytes, None)

    for kw in (dict(logits=None), dict(labels=None), dict(loss=None), dict(ws=None), dict(B=0), dict(Cc=0), dict(H=0), dict(W=0),
               dict(gamma=-0.5), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(red=3), dict(red=-1), dict(dl=p, inv=None)):
        assert focal(**kw) == einval, kw
    assert focal(nbytes=8) == small
