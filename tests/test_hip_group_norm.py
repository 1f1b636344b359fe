"""GroupNorm on the device (csrc/group_norm.hip) against the oracle of tests/group_norm_oracle.py.

The project's standing parity bound: the SAME oracle run in torch float32 on the CPU against its float64 run is the yardstick,
computed here per case and never taken from the device; the device may be at most ``max(4 x yardstick, 2^-23 max|value|)`` away
from float64, per tensor (y, dx, dgamma, dbeta; maxima over the tensor).  Each case runs on data at offset / scale (0, 1),
(100, 1) and (-1000, 0.5): a variance formed as E[x^2] - E[x]^2 in float is off by about 1e-3 at offset 100, thirty times the
yardstick there, so the offset cases separate a right statistic from a wrong one.  The worst device-error-to-bound ratio of
every case is reported with ``report_line``.

The fused ReLU is stated through the device's own mask, because rounding may flip a mask bit next to zero: the fused forward
equals relu(unfused) bit for bit, the fused backward equals the unfused backward fed dy (y > 0) bit for bit, and the float64
backward evaluated with the device's mask stays within the bound, the masks differing only where the float64 pre-activation is
within the y bound of zero."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_norm_oracle as go  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
NAMES = ("y", "dx", "dgamma", "dbeta")
ALL_CASES = range(len(go.CASES))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def bound(yard, value):
    return max(4.0 * yard, ULP * value.abs().max().item())


def maxerr(a, b):
    return (a.detach().cpu().double() - b).abs().max().item()


def ratio(e, b):
    return e / b if b > 0 else (0.0 if e == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def reference(case, content, eps=1e-5, affine=True):
    """Inputs, the float64 results and the float32-against-float64 yardsticks of one case, computed once on the CPU."""
    G = go.CASES[case][4]
    x, gamma, beta, dy = go.make_inputs(case, content)
    if not affine:
        gamma = beta = None
    out = {}
    for dtype in (torch.float64, torch.float32):
        y, _, _, _ = go.forward(x, G, gamma, beta, eps, dtype=dtype)
        assert y.dtype == dtype
        out[dtype] = (y,) + go.backward(x, dy, G, gamma, eps, dtype=dtype)
    yard = {n: (a.double() - b).abs().max().item() for n, a, b in zip(NAMES, out[torch.float32], out[torch.float64])}
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, G=G, yard=yard, **dict(zip(NAMES, out[torch.float64])))


@functools.lru_cache(maxsize=None)
def relu_reference(case):
    """No-offset data under the fused ReLU: the float64 forward (y and the value in front of the ReLU) and the yardsticks of
    the backward, both precisions evaluated with the float64 mask - a yardstick of the arithmetic, free of mask flips."""
    G = go.CASES[case][4]
    x, gamma, beta, dy = go.make_inputs(case, 0)
    y64, pre64, _, _ = go.forward(x, G, gamma, beta, relu=True)
    y32, _, _, _ = go.forward(x, G, gamma, beta, relu=True, dtype=torch.float32)
    mask = pre64 > 0
    b64 = go.backward(x, dy, G, gamma, mask=mask)
    b32 = go.backward(x, dy, G, gamma, mask=mask, dtype=torch.float32)
    yard = {n: (a.double() - b).abs().max().item() for n, a, b in zip(NAMES, (y32,) + b32, (y64,) + b64)}
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, G=G, y=y64, pre=pre64, yard=yard)


def run(dev, x, G, gamma, beta, dy, eps=1e-5, relu=False, needs=(True, True, True)):
    """ops.group_norm and its gradients on the device -> y, dx, dgamma, dbeta (None where not asked for / no parameter)."""
    from weaklysuperviseddl_amd import ops
    xd = x.to(dev).requires_grad_(needs[0])
    gd = None if gamma is None else gamma.to(dev).requires_grad_(needs[1])
    bd = None if beta is None else beta.to(dev).requires_grad_(needs[2])
    y = ops.group_norm(xd, G, gd, bd, eps, relu)
    wrt = [t for t in (xd, gd, bd) if t is not None and t.requires_grad]
    grads = list(torch.autograd.grad(y, wrt, dy.to(dev))) if wrt else []
    res = [grads.pop(0) if (t is not None and t.requires_grad) else None for t in (xd, gd, bd)]
    return (y.detach(),) + tuple(res)


@pytest.mark.parametrize("content", range(len(go.CONTENTS)))
@pytest.mark.parametrize("case", ALL_CASES)
def test_forward_and_backward_against_float64(dev, case, content):
    from conftest import report_line
    r = reference(case, content)
    got = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"])
    worst, lines = 0.0, []
    for n, t in zip(NAMES, got):
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(r[n].shape) and t.is_contiguous()
        err, b = maxerr(t, r[n]), bound(r["yard"][n], r[n])
        lines.append(f"{n} {err:.3e} / {b:.3e}")
        worst = max(worst, ratio(err, b))
    print(f"{go.name_of(case)} data {go.CONTENTS[content]}: " + "; ".join(lines))
    report_line(f"group norm {go.name_of(case)} offset {go.CONTENTS[content][0]:g}: device error / bound at most {worst:.2f}")
    for n, t in zip(NAMES, got):
        assert maxerr(t, r[n]) <= bound(r["yard"][n], r[n]), (n, maxerr(t, r[n]), bound(r["yard"][n], r[n]))


@pytest.mark.parametrize("case", ALL_CASES)
def test_fused_relu_is_the_unfused_pair_bit_for_bit(dev, case):
    """(a) relu=True equals ops.relu(ops.group_norm(...)); (b) its backward equals the unfused backward fed dy (y > 0)."""
    from weaklysuperviseddl_amd import ops
    for content in range(len(go.CONTENTS)):
        r = reference(case, content)
        y, dx, dgamma, dbeta = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"], relu=True)
        plain = ops.group_norm(r["x"].to(dev), r["G"], r["gamma"].to(dev), r["beta"].to(dev))
        assert torch.equal(y, ops.relu(plain)) and y.min().item() >= 0
        masked = r["dy"] * (y > 0).cpu()
        _, dx2, dgamma2, dbeta2 = run(dev, r["x"], r["G"], r["gamma"], r["beta"], masked)
        assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2), content


@pytest.mark.parametrize("case", ALL_CASES)
def test_fused_relu_backward_against_float64_through_the_device_mask(dev, case):
    from conftest import report_line
    r = relu_reference(case)
    G = r["G"]
    y, dx, dgamma, dbeta = run(dev, r["x"], G, r["gamma"], r["beta"], r["dy"], relu=True)
    b_y = bound(r["yard"]["y"], r["y"])
    assert maxerr(y, r["y"]) <= b_y, (maxerr(y, r["y"]), b_y)
    mask = (y > 0).cpu()
    flipped = mask != (r["pre"] > 0)
    n_flip = int(flipped.sum())
    assert n_flip <= 1e-4 * mask.numel(), (n_flip, mask.numel())
    assert n_flip == 0 or r["pre"][flipped].abs().max().item() <= b_y
    want = go.backward(r["x"], r["dy"], G, r["gamma"], mask=mask)
    worst = 0.0
    for n, t, w in zip(NAMES[1:], (dx, dgamma, dbeta), want):
        err, b = maxerr(t, w), bound(r["yard"][n], w)
        worst = max(worst, ratio(err, b))
        assert err <= b, (n, err, b)
    report_line(f"group norm + relu {go.name_of(case)}: {n_flip} of {mask.numel()} mask bits differ from float64; backward error / "
                f"bound at most {worst:.2f}")


def test_a_zero_channel_under_relu_contributes_nothing(dev):
    """gamma = beta = 0 in one channel: y = 0 there, dgamma = dbeta = 0 exactly for it, and dx equals the dx of the same call
    with that channel's upstream gradient zeroed (its mask is empty: it adds nothing to the group's means)."""
    case = 6
    r = reference(case, 1)
    gamma, beta = r["gamma"].clone(), r["beta"].clone()
    gamma[5] = beta[5] = 0.0
    y, dx, dgamma, dbeta = run(dev, r["x"], r["G"], gamma, beta, r["dy"], relu=True)
    assert not y[:, 5].any() and dgamma[5].item() == 0.0 and dbeta[5].item() == 0.0 and dgamma[4].item() != 0.0
    dy0 = r["dy"].clone()
    dy0[:, 5] = 0.0
    _, dx0, _, _ = run(dev, r["x"], r["G"], gamma, beta, dy0, relu=True)
    assert torch.equal(dx, dx0) and torch.isfinite(dx).all()


@pytest.mark.parametrize("case", (2, 7))
def test_without_affine_parameters(dev, case):
    for content in (0, 2):
        r = reference(case, content, affine=False)
        y, dx, dgamma, dbeta = run(dev, r["x"], r["G"], None, None, r["dy"])
        assert dgamma is None and dbeta is None
        for n, t in (("y", y), ("dx", dx)):
            assert maxerr(t, r[n]) <= bound(r["yard"][n], r[n]), (n, content)


@pytest.mark.parametrize("case", (2, 4, 8))
def test_only_the_needed_gradients_and_the_same_bits(dev, case):
    """dx only, the parameters only, one parameter only: each equals the full call bit for bit."""
    r = reference(case, 1)
    args = (dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"])
    for relu in (False, True):
        y, dx, dgamma, dbeta = run(*args, relu=relu)
        y1, dx1, g1, b1 = run(*args, relu=relu, needs=(True, False, False))
        assert torch.equal(y1, y) and torch.equal(dx1, dx) and g1 is None and b1 is None
        _, dx2, g2, b2 = run(*args, relu=relu, needs=(False, True, True))
        assert dx2 is None and torch.equal(g2, dgamma) and torch.equal(b2, dbeta)
        _, dx3, g3, b3 = run(*args, relu=relu, needs=(False, False, True))
        assert dx3 is None and g3 is None and torch.equal(b3, dbeta)
        _, dx4, g4, b4 = run(*args, relu=relu, needs=(True, True, False))
        assert torch.equal(dx4, dx) and torch.equal(g4, dgamma) and b4 is None


def test_strided_views_and_an_odd_storage_offset(dev):
    """A strided view is copied dense: the same bits as the dense call.  A dense view that starts one float into its storage is
    4-byte aligned only and takes the one-float-per-lane kernels although HW % 4 == 0: their sums run in another order, so that
    call is held to the float64 bound, not to the bits.  Gradients land in the views' bases."""
    from weaklysuperviseddl_amd import ops
    r = reference(7, 1)
    x, gamma, beta, dy = (r[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    want_y, want_dx, _, _ = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"], relu=True)
    wide = torch.stack([x, x + 1.0], dim=-1).requires_grad_()
    view = wide[..., 0]
    assert not view.is_contiguous()
    y = ops.group_norm(view, r["G"], gamma, beta, relu=True)
    y.backward(torch.stack([dy, dy], dim=-1)[..., 1])
    assert torch.equal(y, want_y) and torch.equal(wide.grad[..., 0], want_dx) and not wide.grad[..., 1].any()
    flat = torch.zeros(x.numel() + 1, device=dev)
    flat[1:] = x.reshape(-1)
    flat.requires_grad_()
    odd = flat[1:].view_as(x)
    gflat = torch.zeros(dy.numel() + 1, device=dev)
    gflat[1:] = dy.reshape(-1)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    g2, b2 = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y2 = ops.group_norm(odd, r["G"], g2, b2)
    y2.backward(gflat[1:].view_as(dy))
    assert flat.grad[0].item() == 0.0
    for n, t in zip(NAMES, (y2, flat.grad[1:].view_as(x), g2.grad, b2.grad)):
        assert maxerr(t, r[n]) <= bound(r["yard"][n], r[n]), n


def test_more_than_four_dimensions_equal_their_reshape(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(3)
    x5 = (torch.randn(2, 6, 3, 5, 7, generator=g) + 10.0).to(dev).requires_grad_()
    x3 = x5.detach().reshape(2, 6, 105).requires_grad_()
    x2 = torch.randn(4, 6, generator=g).to(dev)
    gamma, beta = torch.randn(6, generator=g).to(dev), torch.randn(6, generator=g).to(dev)
    dy = torch.randn(2, 6, 105, generator=g).to(dev)
    y5, y3 = ops.group_norm(x5, 3, gamma, beta), ops.group_norm(x3, 3, gamma, beta)
    assert tuple(y5.shape) == (2, 6, 3, 5, 7) and torch.equal(y5.reshape(2, 6, 105), y3)
    (d5,), (d3,) = torch.autograd.grad(y5, x5, dy.view_as(y5)), torch.autograd.grad(y3, x3, dy)
    assert torch.equal(d5.reshape(2, 6, 105), d3)
    y2 = ops.group_norm(x2, 2, gamma, beta)                       # (B, C): HW = 1
    want, _, _, _ = go.forward(x2.cpu(), 2, gamma.cpu(), beta.cpu())
    assert tuple(y2.shape) == (4, 6) and maxerr(y2, want) <= 1e-5


@pytest.mark.parametrize("case", (4, 6))
def test_two_calls_give_the_same_bits_and_leave_the_inputs_alone(dev, case):
    r = reference(case, 2)
    xd, gd, bd, dyd = (r[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    from weaklysuperviseddl_amd import ops

    def call():
        xr, gr, br = xd.clone().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
        y = ops.group_norm(xr, r["G"], gr, br, relu=True)
        return (y.detach(),) + torch.autograd.grad(y, (xr, gr, br), dyd)
    first, second = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(xd.cpu(), r["x"]) and torch.equal(gd.cpu(), r["gamma"]) and torch.equal(bd.cpu(), r["beta"])
    assert torch.equal(dyd.cpu(), r["dy"])


@pytest.mark.parametrize("eps", (1e-5, 1e-3))
def test_eps(dev, eps):
    r = reference(2, 0, eps)
    got = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"], eps=eps)
    for n, t in zip(NAMES, got):
        assert maxerr(t, r[n]) <= bound(r["yard"][n], r[n]), (n, eps)
    other = reference(2, 0, 1e-3 if eps == 1e-5 else 1e-5)
    assert maxerr(got[0], other["y"]) > bound(other["yard"]["y"], other["y"])           # (eps matters at this size)


def test_a_constant_group_is_finite(dev):
    """var = 0: rstd = eps^-1/2, y = beta, finite gradients - at a value whose square is far beyond the float32 grid."""
    x = torch.full((2, 4, 5, 6), 1234.5)
    x[1, 2:] = torch.randn(2, 5, 6, generator=torch.Generator().manual_seed(1))
    _, gamma, beta, _ = go.make_inputs(2, 0)
    gamma, beta = gamma[:4].contiguous(), beta[:4].contiguous()
    dy = torch.randn(2, 4, 5, 6, generator=torch.Generator().manual_seed(2))
    y, dx, dgamma, dbeta = run(dev, x, 2, gamma, beta, dy)
    assert all(torch.isfinite(t).all() for t in (y, dx, dgamma, dbeta))
    assert torch.equal(y[0].cpu(), beta.view(4, 1, 1).expand(4, 5, 6)) and torch.equal(y[1, :2].cpu(), y[0, :2].cpu())
    want, _, _, _ = go.forward(x, 2, gamma, beta)
    assert maxerr(y, want) <= 4e-6


def test_a_nan_poisons_its_own_group_only(dev):
    r = reference(2, 0)
    x = r["x"].clone()
    x[1, 3, 2, 4] = float("nan")                      # image 1, group 1 (channels 2, 3)
    y, dx, dgamma, dbeta = run(dev, x, r["G"], r["gamma"], r["beta"], r["dy"])
    bad = torch.zeros(2, 6, dtype=torch.bool)
    bad[1, 2:4] = True
    assert torch.isnan(y.cpu()[bad]).all() and torch.isnan(dx.cpu()[bad]).all()
    assert torch.isfinite(y.cpu()[~bad]).all() and torch.isfinite(dx.cpu()[~bad]).all()
    clean = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"])
    assert torch.equal(y.cpu()[~bad], clean[0].cpu()[~bad]) and torch.equal(dx.cpu()[~bad], clean[1].cpu()[~bad])
    assert torch.isnan(dgamma[2:4]).all() and torch.isfinite(dgamma[:2]).all() and torch.isfinite(dgamma[4:]).all()


def test_a_group_of_one_element(dev):
    """Accepted where torch refuses: y = beta and dx = 0 exactly, dgamma = 0, dbeta = the sum of dy."""
    for shape, G in (((1, 1, 1, 1), 1), ((3, 8, 1, 1), 8), ((5, 4), 4)):
        g = torch.Generator().manual_seed(len(shape))
        x = torch.randn(shape, generator=g) * 0.5 - 1000.0
        C = shape[1]
        gamma, beta, dy = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(shape, generator=g)
        for relu in (False, True):
            y, dx, dgamma, dbeta = run(dev, x, G, gamma, beta, dy, relu=relu)
            want = beta.view((1, C) + (1,) * (len(shape) - 2)).expand(shape)
            want = want.clamp(min=0) if relu else want
            assert torch.equal(y.cpu(), want) and not dx.any() and not dgamma.any()
            m = (want > 0).float() if relu else torch.ones(shape)
            dims = [0] + list(range(2, len(shape)))
            assert maxerr(dbeta, (dy * m).double().sum(dim=dims)) <= 4 * ULP * max(1.0, dy.abs().sum().item())


def test_refusals(dev):
    import ctypes
    from weaklysuperviseddl_amd import ops, lib
    x = torch.randn(2, 6, 4, 4, device=dev)
    w = torch.ones(6, device=dev)
    for bad in (lambda: ops.group_norm(x, 4), lambda: ops.group_norm(x, 0), lambda: ops.group_norm(x, -2),
                lambda: ops.group_norm(x[:0], 2), lambda: ops.group_norm(x[:, :, :0], 2), lambda: ops.group_norm(x[:, :0], 1),
                lambda: ops.group_norm(x.double(), 2), lambda: ops.group_norm(x.cpu(), 2), lambda: ops.group_norm(x, 2, w[:5]),
                lambda: ops.group_norm(x, 2, w, w.cpu()), lambda: ops.group_norm(x, 2, w.double()),
                lambda: ops.group_norm(x, 2, eps=-1e-5), lambda: ops.group_norm(x[0, 0, 0], 1)):
        with pytest.raises(ops.WsdlError):
            bad()
    # the C ABI refuses the same, and a geometry beyond 2^31 - 1 elements or a short workspace, before it launches anything
    L = lib()
    y = torch.empty_like(x)
    stats = torch.empty(2, 4, device=dev, dtype=torch.float64)
    ws = torch.empty(1 << 16, device=dev, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731

    def fwd(B, C, HW, G, eps=1e-5, ws_bytes=ws.numel()):
        return L.wsdl_group_norm_fwd(p(x), None, None, p(y), p(stats[0]), p(stats[1]), B, C, HW, G, eps, 0, p(ws), ws_bytes, None)

    def bwd(B, C, HW, G, relu=0, dx=True, ws_bytes=ws.numel()):
        return L.wsdl_group_norm_bwd(p(x), p(y), None, None, p(stats[0]), p(stats[1]), p(y) if dx else None, None, None, B, C, HW, G,
                                     relu, 0, p(ws), ws_bytes, None)
    assert L.wsdl_group_norm_workspace(2, 6, 16, 2) > 0 and fwd(2, 6, 16, 2) == 0
    for args, word in (((2, 6, 16, 4), "divide"), ((2, 6, 16, 0), "num_groups"), ((0, 6, 16, 2), "empty"), ((2, 6, 0, 2), "empty"),
                       ((2, 1 << 15, 1 << 15, 1), "2^31"), ((1 << 16, 1 << 16, 1, 1), "2^31")):
        assert L.wsdl_group_norm_workspace(*args) == 0, args
        assert fwd(*args) != 0 and word in L.wsdl_last_error().decode(), (args, L.wsdl_last_error())
        assert bwd(*args) != 0 and word in L.wsdl_last_error().decode(), (args, L.wsdl_last_error())
    assert fwd(2, 6, 16, 2, ws_bytes=8) != 0 and "workspace" in L.wsdl_last_error().decode()
    assert bwd(2, 6, 16, 2, ws_bytes=8) != 0 and "workspace" in L.wsdl_last_error().decode()
    assert fwd(2, 6, 16, 2, eps=float("nan")) != 0 and bwd(2, 6, 16, 2, relu=1) != 0 and bwd(2, 6, 16, 2, dx=False) != 0
    assert L.wsdl_group_norm_workspace(1, 1, (1 << 31) - 1, 1) > 0                        # (the largest tensor that is accepted)
    torch.cuda.synchronize()


def test_the_module_is_the_op(dev):
    from weaklysuperviseddl_amd import ops, nn as wnn
    r = reference(7, 1)
    x, dy = r["x"].to(dev), r["dy"].to(dev)
    for relu in (False, True):
        mod = wnn.GroupNorm(r["G"], 32, eps=1e-4, relu=relu).to(dev)
        with torch.no_grad():
            mod.weight.copy_(r["gamma"])
            mod.bias.copy_(r["beta"])
        x1, x2 = x.clone().requires_grad_(), x.clone().requires_grad_()
        g2, b2 = r["gamma"].to(dev).requires_grad_(), r["beta"].to(dev).requires_grad_()
        y1, y2 = mod(x1), ops.group_norm(x2, r["G"], g2, b2, 1e-4, relu)
        y1.backward(dy)
        y2.backward(dy)
        assert torch.equal(y1, y2) and torch.equal(x1.grad, x2.grad) and torch.equal(mod.weight.grad, g2.grad)
        assert torch.equal(mod.bias.grad, b2.grad)
        mod.eval()
        assert torch.equal(mod(x), y1)                               # train and eval are the same function
    bare = wnn.GroupNorm(r["G"], 32, affine=False).to(dev)
    assert torch.equal(bare(x), ops.group_norm(x, r["G"]))


def test_flat_optimiser_receives_the_parameter_gradients_in_place(dev):
    """With a FlatAdam over the module's parameters the backward writes p.grad (a slice of the flat buffer) itself: the same
    bits as the returned gradients; a second backward without zero_grad accumulates to exactly twice that."""
    from weaklysuperviseddl_amd import nn as wnn
    from weaklysuperviseddl_amd.optim import FlatAdam
    r = reference(6, 1)
    x, dy = r["x"].to(dev), r["dy"].to(dev)
    _, want_dx, want_dg, want_db = run(dev, r["x"], r["G"], r["gamma"], r["beta"], r["dy"], relu=True)
    mod = wnn.GroupNorm(r["G"], 32, relu=True).to(dev)
    with torch.no_grad():
        mod.weight.copy_(r["gamma"])
        mod.bias.copy_(r["beta"])
    opt = FlatAdam(list(mod.parameters()), lr=1e-3)
    opt.zero_grad()
    slots = (mod.weight.grad.data_ptr(), mod.bias.grad.data_ptr())
    xr = x.clone().requires_grad_()
    mod(xr).backward(dy)
    assert (mod.weight.grad.data_ptr(), mod.bias.grad.data_ptr()) == slots
    assert mod.weight.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * opt.offsets[0]
    assert torch.equal(mod.weight.grad, want_dg) and torch.equal(mod.bias.grad, want_db) and torch.equal(xr.grad, want_dx)
    mod(x.clone().requires_grad_()).backward(dy)
    assert torch.equal(mod.weight.grad, 2 * want_dg) and torch.equal(mod.bias.grad, 2 * want_db)
    opt.zero_grad()
    mod(x).backward(dy)                                   # (x needs no gradient: the two-launch backward)
    assert torch.equal(mod.weight.grad, want_dg) and torch.equal(mod.bias.grad, want_db)


def test_launch_plan_holds_forward_and_backward(dev):
    """forward + autograd.grad wrt x, weight and bias as a plan: six kernels - chunk statistics, one wave per group, apply;
    chunk sums, one wave per group and per channel, dx - bit-identical to the eager call, replayed on new contents, and a new
    recording for another num_groups."""
    from weaklysuperviseddl_amd import ops, plan
    r = reference(7, 1)
    x, gamma, beta = (r[k].to(dev).requires_grad_() for k in ("x", "gamma", "beta"))
    dy = r["dy"].to(dev)

    def step(G):
        y = ops.group_norm(x, G, gamma, beta, relu=True)
        return (y,) + torch.autograd.grad(y, (x, gamma, beta), dy)
    p, recorded = plan.record(step, 4)
    eager = step(4)
    assert p.stats["kernels"] == 6 and p.stats["memsets"] == 0
    assert all(torch.equal(a, b) for a, b in zip(recorded, eager))
    first = [t.clone() for t in recorded]
    with torch.no_grad():
        x.copy_((x * 0.5 + x.flip(-1)).contiguous())
        gamma.copy_((gamma.flip(0) * 1.5).contiguous())
        beta.copy_((beta - 0.25).contiguous())
        dy.copy_(dy.flip(-2).contiguous())
    p.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in recorded]
    fresh = step(4)
    assert all(torch.equal(a, b) for a, b in zip(replayed, fresh)) and not any(torch.equal(a, b) for a, b in zip(replayed, first))
    p8, rec8 = plan.record(step, 8)
    assert p8.stats["kernels"] == 6 and all(torch.equal(a, b) for a, b in zip(rec8, step(8)))
    assert not torch.equal(rec8[0], fresh[0])


def _trunk(dev):
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM
    torch.manual_seed(0)
    model = FrozenResNetCAM(37)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return model.to(dev).eval()


def _stages(trunk, x):
    with torch.no_grad():
        f0 = trunk.layer0(x)
        f1 = trunk.layer1(f0)
        f2 = trunk.layer2(f1)
        f3 = trunk.layer3(f2)
        f4 = trunk.layer4(f3)
    return f0, f1, f2, f3, f4


def test_boundary_net_with_and_without_the_norm(dev):
    """A 64 x 64 image: logits (B,1,16,16) equal to the composition of the ops bit for bit, with GroupNorm and - the network as
    it was - without; finite gradients on the six convolutions and the ten GroupNorm tensors, none on the trunk."""
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import BoundaryNet
    trunk = _trunk(dev)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    feats = _stages(trunk, x)
    size = tuple(feats[1].shape[-2:])
    for norm in (None, "group"):
        torch.manual_seed(1)
        net = BoundaryNet(trunk, norm=norm).to(dev).train()
        if norm:
            g = torch.Generator().manual_seed(9)
            with torch.no_grad():
                for gn in net._norms():
                    gn.weight.copy_(torch.rand(32, generator=g) + 0.5)
                    gn.bias.copy_(torch.randn(32, generator=g) * 0.1)
        logits = net(x)
        assert tuple(logits.shape) == (2, 1, 16, 16) and torch.isfinite(logits).all() and not net.trunk.training
        maps = []
        for i, f in enumerate(feats):
            m = getattr(net, f"fc_edge{i + 1}")(f)
            if norm:
                gn = getattr(net, f"gn_edge{i + 1}")
                m = ops.group_norm(m, 4, gn.weight, gn.bias, 1e-5, True)
            else:
                m = ops.relu(m)
            maps.append(m if tuple(m.shape[-2:]) == size else ops.bilinear_resize(m, size))
        assert torch.equal(logits, net.fc_edge6(ops.concat_channels(maps))), norm
        logits.backward(torch.randn(2, 1, 16, 16, generator=torch.Generator().manual_seed(6)).to(dev))
        with_grad = sorted(k for k, p in net.named_parameters() if p.grad is not None)
        want = [f"fc_edge{i}.weight" for i in range(1, 7)] + ["fc_edge6.bias"]
        if norm:
            want += [f"gn_edge{i}.{n}" for i in range(1, 6) for n in ("weight", "bias")]
        assert with_grad == sorted(want)
        for k, p in net.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all(), k
                if k.startswith("gn_edge") and k.endswith("weight"):
                    assert p.grad.abs().max().item() > 0, k


def test_train_boundary_net_with_the_normalised_head(dev):
    import math
    from weaklysuperviseddl_amd.TraditionalModel import BoundaryNet, train_boundary_net
    trunk = _trunk(dev)
    torch.manual_seed(2)
    net = BoundaryNet(trunk, norm="group")
    before = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
    g = torch.Generator().manual_seed(8)
    loader = [(torch.rand(2, 3, 64, 64, generator=g), None) for _ in range(2)]
    ramp = torch.linspace(0, 1, 64).view(1, 1, 64).expand(2, 64, 64).contiguous()
    history = train_boundary_net(net, loader, [ramp, ramp.transpose(1, 2).contiguous()], lo=0.45, hi=0.55, radius=5, device=dev, log=None)
    assert len(history) == 1 and math.isfinite(history[0]) and not net.training
    moved = [k for k, p in net.named_parameters() if not torch.equal(p.detach().cpu(), before[k])]
    print(f"loss {history[0]:.6e}; moved: {moved}")
    assert not any(k.startswith("trunk.") for k in moved)
    for k, p in net.named_parameters():
        if not k.startswith("trunk."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
