"""The weight gradients' producer path against float64: the channel-resident BatchNorm kernels publish one maximum per channel
(``bn_train_fwd`` of y, ``bn_train_bwd`` of dx) and the backward writes dx a second time as the fp16 (high, low) rows the
producing convolution's weight gradient reads; ``ops.conv2d_wgrad`` hands them to ``wsdl_conv2d_wgrad_ex``, which then runs the
channel-scaled kernels and skips ``dy_split16_kernel``.  The training step takes this path by default.

Every case is producer -> consumer through ``ops``: x = ``bn_train_fwd(relu=True)`` of a random tensor, dY = ``bn_train_bwd`` of a
random gradient, dW = ``conv2d_wgrad(x, dY, ..., x_camax=, dy_camax=, dy_presplit=)``.  The reference is
``torch.nn.grad.conv2d_weight`` in float64 on the CPU applied to the DEVICE's x and dY, so only the weight-gradient kernels and
their scales are under test (no ReLU-mask flips; no element is left out of any comparison).

The error measure is the project's (tests/test_hip_ops.py::test_wgrad_channel_scales...): per row (Cout) and per column (Cin) of
dW relative to that row's / column's own reference maximum, the worst of all rows and columns.  Bounds: <= 1e-4 everywhere (the
bound the project asserts for these kernels); on unit data <= 1.5 x the per-tensor-scale result + 1e-7; on graded data <= the
per-tensor-scale result.  A row / column whose reference is all zero must be exactly zero.

The second half holds the tests of state that rides beside tensors: per-channel maxima and pre-split rows carry the version of
the tensor they describe (``ops.camax_of``) and are dropped after an in-place edit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- geometry
# (B, Cin, H, W, Cout, k, stride, dilation): x is (B, Cin, H, W), dY (B, Cout, OH, OW); padding (k // 2) * dilation.
# kernel: the trace's kernel name; src: where the kernel takes dY from; cs: per-channel scales in use;
# fwd / bwd: threads of the channel-resident BatchNorm form that produces x / dY (0: the two-pass form, no maxima; 1025: the
# forward's 1024 threads x 16 float4).
PRE, RAW, SPLIT = "dY pre-split by its producer", "dyraw", "dy_split16"
GEOMS = {
    "1-direct-dyraw":        ((2, 128, 16, 32, 128, 3, 1, 4), "wgrad_split16d", RAW, 1, 1024, 1024),
    "2-direct-presplit":     ((2, 256, 16, 32, 128, 3, 1, 4), "wgrad_split16d", PRE, 1, 1024, 1024),
    "3-staged-d1":           ((2, 128, 16, 32, 128, 3, 1, 1), "wgrad_split16", PRE, 1, 1024, 1024),
    "3-staged-d2":           ((2, 128, 16, 32, 128, 3, 1, 2), "wgrad_split16", PRE, 1, 1024, 1024),
    "4-bwd256":              ((2, 256, 16, 32, 384, 3, 1, 4), "wgrad_split16d", PRE, 1, 1024, 256),
    "5-bwd512-staged":       ((3, 128, 96, 64, 128, 3, 1, 1), "wgrad_split16", PRE, 1, 512, 512),
    "5-bwd512-direct":       ((3, 256, 96, 64, 128, 3, 1, 4), "wgrad_split16d", PRE, 1, 512, 512),
    "6-stride2":             ((2, 128, 32, 64, 128, 3, 2, 1), "wgrad_split16", PRE, 1, 1024, 1024),
    "7-ow24":                ((2, 128, 16, 24, 128, 3, 1, 4), "wgrad_split16", PRE, 1, 1024, 1024),
    "8-p144":                ((1, 128, 12, 12, 128, 3, 1, 1), "wgrad_split16", SPLIT, 1, 1024, 1024),
    "9-hw81":                ((2, 128, 9, 9, 128, 3, 1, 1), "wgrad_split16", SPLIT, 0, 0, 0),
    "10-1x1-dyraw":          ((2, 256, 16, 32, 128, 1, 1, 1), "wgrad_split16d", RAW, 1, 1024, 1024),
    "11-1x1-wide":           ((2, 1408, 8, 32, 128, 1, 1, 1), "wgrad_split16d", PRE, 1, 256, 1024),
    "12-mixed-staged":       ((9, 128, 64, 64, 128, 3, 1, 1), "wgrad_split16", SPLIT, 1, 1025, 0),
    "12-mixed-dyraw":        ((9, 128, 64, 64, 128, 1, 1, 1), "wgrad_split16d", RAW, 1, 1025, 0),
}
VARIANT_GEOMS = ("2-direct-presplit", "3-staged-d1", "3-staged-d2", "4-bwd256")
MODE_GEOMS = ("1-direct-dyraw", "2-direct-presplit", "4-bwd256", "5-bwd512-staged")        # case 1 + one per backward form
ACC_GEOMS = ("1-direct-dyraw", "2-direct-presplit", "3-staged-d1")    # one per kernel form: direct + fp32 dY, direct + rows, staged


def _bn_form(C, n, HW, backward):
    """Threads of the channel-resident BatchNorm kernel for C channels of n = B * HW values (``resident_threads`` in
    csrc/norm_pool.hip with the default options; checked against ``wsdl_bn_channel_resident`` wherever it is used)."""
    if C < 64 or HW % 4:
        return 0
    if n <= 16384 and C <= (256 if backward else 512):
        return 1024
    if n <= 16384:
        return 256
    if n <= 32768:
        return 512
    if not backward and n <= 65536:
        return 1025
    return 0


def _out_hw(geom):
    B, Cin, H, W, Cout, k, s, d = geom
    pad = (k // 2) * d
    return (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1, pad


def _chan_max(t):
    return t.abs().amax(dim=(0, 2, 3)).contiguous()


def _plain(t):
    """The same values in a tensor without the producer's attributes."""
    return torch.empty_like(t).copy_(t)


_chains = {}


def _chain(dev, name, data="unit"):
    """The producers of one case, run once per (geometry, data) and shared read-only by the tests: x with its per-channel
    maxima, dY (mode 2: the ReLU mask recomputed from the convolution output) with maxima and rows, and what the other two
    mask modes need."""
    from weaklysuperviseddl_amd import ops
    key = (name, data)
    if key in _chains:
        return _chains[key]
    geom = GEOMS[name][0]
    B, Cin, H, W, Cout, k, s, d = geom
    OH, OW, pad = _out_hw(geom)
    g = torch.Generator(device=dev).manual_seed(1000 + sum(geom) + len(data))
    xin = torch.randn(B, Cin, H, W, device=dev, generator=g)
    gx, bx = torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g) * 0.1
    conv_out = torch.randn(B, Cout, OH, OW, device=dev, generator=g)
    dy = torch.randn(B, Cout, OH, OW, device=dev, generator=g)
    gamma, beta = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g) * 0.1
    if data == "graded":            # channels of dY 2^-30 below and 2^20 above the rest: where one scale per tensor loses bits
        gamma[::7] *= 2.0 ** -30
        gamma[3::7] *= 2.0 ** 20
    elif data == "dead":            # one dY channel exactly zero (maximum 0), one x channel all zero behind its ReLU
        gamma[9] = 0.0
        bx[5] = -100.0
    x, _m, _i = ops.bn_train_fwd(xin, gx, bx, torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev), 0.1, 1e-5, relu=True)
    y, mean, invstd, bits = ops.bn_train_fwd(conv_out, gamma, beta, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev),
                                             0.1, 1e-5, relu=True, want_mask=True, mask_if=True)
    wshape = (Cout, Cin, k, k)
    psb = ops.wgrad_presplit_bytes(tuple(x.shape), wshape, s, pad, d)
    dx, _, _, _ = ops.bn_train_bwd(conv_out, dy, None, gamma, mean, invstd, True, False, beta=beta, presplit_bytes=psb)
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), wshape, dx.double().cpu(), s, pad, d)
    c = dict(geom=geom, wshape=wshape, s=s, pad=pad, d=d, x=x, dx=dx, psb=psb, ref=ref, conv_out=conv_out, dy=dy, gamma=gamma,
             beta=beta, mean=mean, invstd=invstd, y=y, bits=bits, P=B * OH * OW, OHW=OH * OW)
    _chains[key] = c
    return c


def _errors(dw, ref, floor=0.0):
    """(worst row error, worst column error) of dW against float64, each relative to the row's / column's own reference
    maximum.  Rows / columns whose reference maximum is <= ``floor`` are not measured; where it is 0, dW must be exactly 0."""
    e = (dw.double().cpu() - ref).abs()
    out = []
    for dims in ((1, 2, 3), (0, 2, 3)):
        ee, mm = e.amax(dim=dims), ref.abs().amax(dim=dims)
        assert bool((ee[mm == 0] == 0).all()), "a row / column whose reference is all zero is not exactly zero"
        live = mm > floor
        out.append((ee[live] / mm[live]).max().item() if bool(live.any()) else 0.0)
    return tuple(out)


def _traced_wgrad(ops, *args, **kw):
    ops.launch_trace(True)
    try:
        ops.last_launches()
        dw = ops.conv2d_wgrad(*args, **kw)
        trace = ops.last_launches()
    finally:
        ops.launch_trace(False)
    return dw, trace


def _check_trace(trace, kernel, src, cs):
    entries = [e.strip() for e in trace.split(";")]
    launch = [e for e in entries if e.startswith("wgrad_split16")]
    assert len(launch) == 1, trace
    assert launch[0].split(" ")[0] == kernel, trace
    assert f" cs={cs} " in launch[0], trace
    assert [e for e in entries if e in (PRE, RAW, SPLIT)] == [src], trace


def _producer_kwargs(ops, c):
    """What the nodes of the training step hand ``conv2d_wgrad``: the operands' published maxima and dY's rows."""
    x_camax = ops.camax_of(c["x"])
    dy_camax, rows = ops.camax_of(c["dx"], presplit=True)
    return dict(x_camax=x_camax, dy_camax=dy_camax, dy_presplit=rows)


def _check_case(dev, name, data):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.ops import lib
    geom, kernel, src, cs, fwd_form, bwd_form = GEOMS[name]
    B, Cin, H, W, Cout, k, s, d = geom
    c = _chain(dev, name, data)
    x, dx, wshape, pad, ref = c["x"], c["dx"], c["wshape"], c["pad"], c["ref"]
    # the BatchNorm forms this case is listed for are the ones the library runs
    assert _bn_form(Cin, B * H * W, H * W, False) == fwd_form and _bn_form(Cout, c["P"], c["OHW"], True) == bwd_form
    assert bool(lib().wsdl_bn_channel_resident(B, Cin, H * W, 0)) == (fwd_form != 0)
    assert bool(lib().wsdl_bn_channel_resident(B, Cout, c["OHW"], 1)) == (bwd_form != 0)
    # (a) the published maxima are exact, wherever the form is channel-resident
    for t, form in ((x, fwd_form), (dx, bwd_form)):
        cam = ops.camax_of(t)
        assert (cam is not None) == (form != 0)
        if cam is not None:
            assert torch.equal(cam, _chan_max(t))
    # (b) pre-split rows
    rows = ops.camax_of(dx, presplit=True)[1]
    assert (rows is not None) == (c["psb"] > 0 and c["P"] % 32 == 0 and bwd_form != 0)
    assert (rows is not None) == (src == PRE)
    assert torch.isfinite(x).all() and torch.isfinite(dx).all()
    # (c) the launch the producer path takes
    dw, trace = _traced_wgrad(ops, x, dx, wshape, s, pad, d, **_producer_kwargs(ops, c))
    _check_trace(trace, kernel, src, cs)
    assert torch.isfinite(dw).all()
    # (d) bit equality with the pre-pass on a plain copy (pins the contents of the rows); needs maxima of dY on both sides
    xp, dxp = _plain(x), _plain(dx)
    if ops.camax_of(dx) is not None:
        xa = _chan_max(x)
        dw_both = ops.conv2d_wgrad(x, dx, wshape, s, pad, d, x_camax=xa, dy_camax=ops.camax_of(dx), dy_presplit=rows)
        ops.set_option("wgrad_chan_scale", 1)
        try:
            dw_prepass, ptrace = _traced_wgrad(ops, xp, dxp, wshape, s, pad, d, x_camax=xa)
        finally:
            ops.set_option("wgrad_chan_scale", 0)
        assert PRE not in ptrace and " cs=1 " in ptrace, ptrace
        assert torch.equal(dw_both, dw_prepass)
        if ops.camax_of(x) is not None:
            assert torch.equal(dw_both, dw)             # (the published maxima of x are the measured ones: (a))
    # (e) against float64, and against one scale per tensor
    dw_tensor, ttrace = _traced_wgrad(ops, xp, dxp, wshape, s, pad, d)
    assert " cs=0 " in ttrace and PRE not in ttrace, ttrace
    row, col = _errors(dw, ref)
    trow, tcol = _errors(dw_tensor, ref)
    e_new, e_tensor = max(row, col), max(trow, tcol)
    print(f"{name} {data}: row {row:.3e} col {col:.3e}; per-tensor row {trow:.3e} col {tcol:.3e}")
    report_line(f"weight gradient, producer path {name} {geom} {data}: worst row / column vs float64 {row:.1e} / {col:.1e} "
                f"(one scale per tensor: {trow:.1e} / {tcol:.1e}) [{launch_of(trace)}]")
    assert e_new <= BOUND, (name, data, row, col)
    if data == "graded":
        assert e_new <= e_tensor, (name, data, e_new, e_tensor)
        assert row <= trow, (name, data, row, trow)                 # dY's channels are the graded ones: the rows of dW
    else:
        assert e_new <= 1.5 * e_tensor + 1e-7, (name, data, e_new, e_tensor)
    if data == "dead":
        assert torch.equal(ops.camax_of(dx)[9], torch.zeros((), device=dev)) and not bool(dx[:, 9].any())
        assert torch.equal(ops.camax_of(x)[5], torch.zeros((), device=dev)) and not bool(x[:, 5].any())
        assert not bool(dw[9].any()) and not bool(dw[:, 5].any())
    return dw


def launch_of(trace):
    return "; ".join(e.strip() for e in trace.split(";") if e.strip().startswith("wgrad_split16") or e.strip() in (PRE, RAW, SPLIT))


@pytest.mark.parametrize("name", list(GEOMS))
def test_producer_path_geometries_against_float64(dev, name):
    """Every combination of weight-gradient kernel (direct-fragment / LDS-staged), dY source (fp32 read, rows written by the
    BatchNorm backward, the split pass) and BatchNorm form (forward 1024 x 4, 256, 512, 1024 x 16; backward 1024 x 4, 256, 512;
    the two-pass form without maxima), at stride 2, OW % 32 != 0, P % 32 != 0, HW % 4 != 0, 1x1 below and above the fp32-dY limit,
    and per-channel x with per-tensor dY: maxima exact, the launch as listed, bit-equal to the pre-pass, within the bounds."""
    _check_case(dev, name, "unit")


@pytest.mark.parametrize("data", ["graded", "dead"])
@pytest.mark.parametrize("name", VARIANT_GEOMS)
def test_producer_path_on_graded_and_dead_channels(dev, name, data):
    """graded: every 7th channel of dY 2^-30 below and another set 2^20 above the rest - each keeps its accuracy, which one scale
    per tensor does not give.  dead: a dY channel that is exactly zero (gamma = 0, maximum 0) and an x channel that is all zero
    behind its ReLU (beta = -100): their rows / columns of dW are exactly zero, everything is finite."""
    _check_case(dev, name, data)


@pytest.mark.parametrize("name", MODE_GEOMS)
def test_mask_modes_write_the_same_dx_maxima_and_rows(dev, name):
    """The ReLU mask from the forward's bits (mode 3) and from the forward output (mode 1) instead of recomputed from the
    convolution output (mode 2): the three masks are the same function of the same fused multiply-add, so dx, its per-channel maxima
    and its pre-split rows are the same bits."""
    from weaklysuperviseddl_amd import ops
    c = _chain(dev, name)
    assert c["bits"] is not None
    args = (c["gamma"], c["mean"], c["invstd"], True, False)
    ref_cam, ref_rows = ops.camax_of(c["dx"], presplit=True)
    assert ref_cam is not None
    for kw in (dict(y=None, relu_mask=c["bits"]), dict(y=c["y"])):
        dx, _, _, _ = ops.bn_train_bwd(c["conv_out"], c["dy"], kw.pop("y"), *args, presplit_bytes=c["psb"], **kw)
        cam, rows = ops.camax_of(dx, presplit=True)
        assert torch.equal(dx, c["dx"])
        assert cam is not None and torch.equal(cam, ref_cam)
        assert (rows is None) == (ref_rows is None)
        if rows is not None:
            # the fp16 rows are [P / 32][Cout][128 bytes] at the front of the buffer (it is sized for the wider rows of the
            # bf16 kernel; the rest is never written or read)
            used = c["P"] // 32 * c["geom"][4] * 128
            assert used <= rows.numel() == ref_rows.numel()
            assert torch.equal(rows[:used], ref_rows[:used])


@pytest.mark.parametrize("name", ACC_GEOMS)
def test_producer_path_accumulates_into_a_prefilled_gradient(dev, name):
    """accumulate=True: out = prefill + dW, within the same bound of float64 (prefill of dW's own size)."""
    from weaklysuperviseddl_amd import ops
    c = _chain(dev, name)
    g = torch.Generator(device=dev).manual_seed(5)
    scale = c["ref"].abs().max().item()
    prefill = torch.randn(c["wshape"], device=dev, generator=g) * scale
    out = prefill.clone()
    _, trace = _traced_wgrad(ops, c["x"], c["dx"], c["wshape"], c["s"], c["pad"], c["d"], out=out, accumulate=True,
                             **_producer_kwargs(ops, c))
    _check_trace(trace, *GEOMS[name][1:4])
    row, col = _errors(out, prefill.double().cpu() + c["ref"])
    assert max(row, col) <= BOUND, (name, row, col)
    fresh = ops.conv2d_wgrad(c["x"], c["dx"], c["wshape"], c["s"], c["pad"], c["d"], **_producer_kwargs(ops, c))
    assert not torch.equal(out, fresh)


PLANTED = [2.0 ** -20, 1.0, 2.0 ** 15, 2.0 ** 20, float(torch.nextafter(torch.tensor(2.0 ** 15), torch.tensor(0.0))), 0.0, 1e-40]


def _plant(t, offset):
    """Channel c of ``t`` (on the host) scaled so that its maximum is PLANTED[(c + offset) % 7]; returns the tensor, the planted
    values and their indices into PLANTED."""
    C = t.shape[1]
    kind = (torch.arange(C) + offset) % len(PLANTED)
    want = torch.tensor(PLANTED, dtype=torch.float32)[kind]
    t = t / t.abs().amax(dim=(0, 2, 3), keepdim=True)               # every channel's maximum is exactly 1
    return t * want.view(1, C, 1, 1), want, kind


def test_hand_fed_maxima_at_powers_of_two_zero_and_subnormal(dev):
    """No producer: ``x_camax`` / ``dy_camax`` computed by torch, each channel's maximum planted - exactly 2^k (k = -20, 0, 15,
    20: the edges of the power-of-two scale's binade), the float just below 2^15, 0, and 1e-40 (a channel of subnormals only).
    Everything is finite; every row / column whose reference maximum is >= 2^-100 is within the bound - which leaves out only
    what the subnormal channel alone decides; zero channels give exact zeros."""
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    geom, kernel, _src, _cs, _f, _b = GEOMS["3-staged-d1"]
    B, Cin, H, W, Cout, k, s, d = geom
    OH, OW, pad = _out_hw(geom)
    g = torch.Generator().manual_seed(77)
    xh, wx, kx = _plant(torch.relu(torch.randn(B, Cin, H, W, generator=g)), 0)
    dyh, wy, ky = _plant(torch.randn(B, Cout, OH, OW, generator=g), 3)
    assert wx[6] > 0 and wx[6] < 2.0 ** -126 and wx[5] == 0                 # (the host keeps the subnormal)
    x, dy = xh.to(dev), dyh.to(dev)
    xa, dya = _chan_max(x), _chan_max(dy)
    assert torch.equal(xa.cpu(), wx) and torch.equal(dya.cpu(), wy), "the planted maxima arrived on the device as planted"
    wshape = (Cout, Cin, k, k)
    ref = torch.nn.grad.conv2d_weight(xh.double(), wshape, dyh.double(), s, pad, d)
    dw, trace = _traced_wgrad(ops, x, dy, wshape, s, pad, d, x_camax=xa, dy_camax=dya)
    _check_trace(trace, kernel, SPLIT, 1)
    assert torch.isfinite(dw).all()
    row, col = _errors(dw, ref, floor=2.0 ** -100)
    report_line(f"weight gradient, hand-fed channel maxima {geom}: worst row / column vs float64 {row:.1e} / {col:.1e}")
    assert max(row, col) <= BOUND, (row, col)
    # the subnormal channels are the only ones below the floor
    rmax, cmax = ref.abs().amax(dim=(1, 2, 3)), ref.abs().amax(dim=(0, 2, 3))
    assert torch.equal((rmax > 0) & (rmax < 2.0 ** -100), ky == 6) and torch.equal(rmax == 0, ky == 5)
    assert torch.equal((cmax > 0) & (cmax < 2.0 ** -100), kx == 6) and torch.equal(cmax == 0, kx == 5)
    assert not bool(dw[(ky == 5).to(dev)].any()) and not bool(dw[:, (kx == 5).to(dev)].any())


# ------------------------------------------------------------------------------------------ state that rides beside tensors
class _Recorder:
    """``ops.conv2d_wgrad`` wrapped: keeps copies of the operands and what came with them (the nodes' backward runs on autograd's
    thread and calls it through the module)."""

    def __init__(self, ops, monkeypatch):
        self.calls = []
        orig = ops.conv2d_wgrad

        def wrapped(x, dy, wshape, stride, pad, dil, **kw):
            self.calls.append(dict(x=x.detach().clone(), dy=dy.detach().clone(), wshape=tuple(wshape), geo=(stride, pad, dil),
                                   x_camax=kw.get("x_camax") is not None, dy_camax=kw.get("dy_camax") is not None,
                                   rows=kw.get("dy_presplit")))
            return orig(x, dy, wshape, stride, pad, dil, **kw)
        monkeypatch.setattr(ops, "conv2d_wgrad", wrapped)


def _node(dev, cin, cout, k, d, seed, stride=1):
    from weaklysuperviseddl_amd import nn as wnn
    torch.manual_seed(seed)
    conv = wnn.Conv2d(cin, cout, k, stride=stride, padding=(k // 2) * d, dilation=d).to(dev)
    bn = wnn.BatchNorm2d(cout).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(cout, device=dev) + 0.5)
        bn.bias.copy_(torch.randn(cout, device=dev) * 0.1)
    return conv, bn


def test_an_in_place_edit_of_x_drops_its_channel_maxima(dev, monkeypatch):
    """conv -> BatchNorm -> ReLU output (carries per-channel maxima), one channel multiplied by 64 in place, then a train-mode
    conv -> BatchNorm node whose weight a FlatAdam owns: the weight gradient must be that of the EDITED tensor.  With the stale
    maxima the channel overflows the fp16 pieces (scaled to 2^20 instead of below 2^15): inf / NaN in dW."""
    from weaklysuperviseddl_amd import nn as wnn, ops
    from weaklysuperviseddl_amd.optim import FlatAdam
    g = torch.Generator(device=dev).manual_seed(31)
    x0 = torch.randn(2, 128, 16, 32, device=dev, generator=g)
    conv0, bn0 = _node(dev, 128, 128, 3, 1, 1)
    conv1, bn1 = _node(dev, 128, 128, 3, 1, 2)
    opt = FlatAdam([conv1.weight, bn1.weight, bn1.bias])
    with torch.no_grad():
        y = wnn.conv_bn(x0, conv0, bn0, True)
    assert getattr(y, "_wsdl_camax", None) is not None, "the producer published per-channel maxima"
    y[:, 3].mul_(64.0)
    rec = _Recorder(ops, monkeypatch)
    out = wnn.conv_bn(y, conv1, bn1, False)
    out.backward(torch.randn(out.shape, device=dev, generator=g))
    ops.join_side_stream(dev)
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    call = rec.calls[0]
    assert torch.equal(call["x"], y) and call["dy_camax"] and call["rows"] is not None
    dw = conv1.weight.grad
    assert torch.isfinite(dw).all(), f"{int((~torch.isfinite(dw)).sum())} of {dw.numel()} weight-gradient values are not finite"
    ref = torch.nn.grad.conv2d_weight(y.double().cpu(), call["wshape"], call["dy"].double().cpu(), *call["geo"])
    row, col = _errors(dw, ref)
    assert max(row, col) <= BOUND, (row, col)
    assert not call["x_camax"], "the maxima of the tensor as it was before the edit were handed to the weight gradient"
    del opt


def test_an_in_place_edit_of_dy_drops_its_maxima_and_pre_split_rows(dev):
    """dx from the BatchNorm backward with pre-split rows, then ``dx.mul_(2)``: the rows still hold the old values - a weight
    gradient that reads them is half of what it should be, with no NaN to notice.  Handed the tensor's own maxima,
    ``conv2d_wgrad`` checks their version, drops them and the rows, and measures the tensor again."""
    from weaklysuperviseddl_amd import ops
    c = _chain(dev, "3-staged-d1")
    x = c["x"]
    dx, _, _, _ = ops.bn_train_bwd(c["conv_out"], c["dy"], None, c["gamma"], c["mean"], c["invstd"], True, False, beta=c["beta"],
                                   presplit_bytes=c["psb"])
    assert getattr(dx, "_wsdl_presplit", None) is not None
    dx.mul_(2.0)
    dw, trace = _traced_wgrad(ops, x, dx, c["wshape"], c["s"], c["pad"], c["d"], dy_camax=dx._wsdl_camax)
    ref = 2.0 * c["ref"]                                  # (dx is the shared chain's, doubled: exact in float64)
    assert torch.equal(dx, 2.0 * c["dx"])
    row, col = _errors(dw, ref)
    hrow, hcol = _errors(dw, c["ref"])
    assert max(hrow, hcol) > 0.4, "the result is the gradient of the tensor as it was before the edit (stale pre-split rows)"
    assert max(row, col) <= BOUND, (row, col)
    assert PRE not in trace and SPLIT in trace, trace
    assert ops.camax_of(dx) is None and ops.camax_of(dx, presplit=True) == (None, None)
    assert ops.camax_of(c["dx"]) is not None              # the untouched tensor keeps its own


def test_nodes_hand_each_convolution_its_own_pre_split_rows(dev, monkeypatch):
    """Two train-mode conv -> BatchNorm nodes under a FlatAdam: the weight gradients with the rows written by the BatchNorm
    backward equal those with ``ops.DY_PRESPLIT`` off (dY split by a pass of its own, same per-channel scales) bit for bit - each
    node's rows belong to its own convolution."""
    from weaklysuperviseddl_amd import nn as wnn, ops
    from weaklysuperviseddl_amd.optim import FlatAdam
    g = torch.Generator(device=dev).manual_seed(41)
    x0 = torch.randn(2, 128, 16, 32, device=dev, generator=g)
    r = torch.randn(2, 256, 16, 32, device=dev, generator=g)
    rec = _Recorder(ops, monkeypatch)
    old = (ops.DY_PRESPLIT[0], ops.CHAN_AMAX[0])
    grads = {}
    try:
        for rows_on in (True, False):
            ops.DY_PRESPLIT[0], ops.CHAN_AMAX[0] = rows_on, True
            conv1, bn1 = _node(dev, 128, 128, 3, 1, 3)
            conv2, bn2 = _node(dev, 128, 256, 3, 2, 4)
            opt = FlatAdam([conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias])
            del rec.calls[:]
            out = wnn.conv_bn(wnn.conv_bn(x0, conv1, bn1, True), conv2, bn2, True)
            out.backward(r)
            ops.join_side_stream(dev)
            torch.cuda.synchronize()
            assert [c["wshape"] for c in rec.calls] == [(256, 128, 3, 3), (128, 128, 3, 3)]
            assert all(c["dy_camax"] and (c["rows"] is not None) == rows_on for c in rec.calls)
            assert rec.calls[0]["x_camax"] and not rec.calls[1]["x_camax"]       # conv2 reads bn1's output, conv1 the input
            if rows_on:
                assert rec.calls[0]["rows"].data_ptr() != rec.calls[1]["rows"].data_ptr()
                assert rec.calls[0]["rows"].numel() == 2 * rec.calls[1]["rows"].numel() > 0      # 256 and 128 channels of rows
            grads[rows_on] = (conv1.weight.grad.clone(), conv2.weight.grad.clone())
            assert all(torch.isfinite(t).all() and bool(t.any()) for t in grads[rows_on])
            del opt
    finally:
        ops.DY_PRESPLIT[0], ops.CHAN_AMAX[0] = old
    assert torch.equal(grads[True][0], grads[False][0]) and torch.equal(grads[True][1], grads[False][1])
