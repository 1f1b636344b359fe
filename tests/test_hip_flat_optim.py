"""The flat optimiser on the device (csrc/flat_optim.hip, optim.FlatAdam / FlatAdamW / FlatSGD) against the float64 oracle of
tests/flat_optim_oracle.py, which tests/test_flat_optim.py holds against live torch.

Bounds are the project's: 1e-5 of max|ref| for the optimiser state (the Adam bound of tests/test_hip_small_ops.py) and ULP4 =
4 fp32 ulps for the norm, whose squares and sums are all taken in double - what is left is one rounding to float.  Sizes come
from the kernels' own grid constants: the norm runs a FIXED grid of ``wsdl_grad_norm_partials()`` workgroups of 256 threads
with 16-byte loads, four loads in flight per thread; the step kernel caps its grid at 8192 workgroups.

The hyper-parameters reach the kernels as float32 (``hyper_dev``), so the oracle starts from their float32 values
(``FlatOracle.as_kernel_reads``), exactly as it starts from the float32 parameters and gradients: with beta2 = 0.999 the
float32 of it makes 1 - beta2 differ from 0.001 by 1.3e-5 of itself, which is a property of the INPUT (the default Adam launch
reads the same float), not rounding inside the step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_optim_oracle as O  # noqa: E402

# Every test that takes the `dev` fixture MUST carry @gpu (see tests/test_hip_small_ops.py)
gpu = pytest.mark.gpu

ULP4 = 4 * 2.0 ** -23           # 4 fp32 ulps of max|ref|, relative
STATE_TOL = 1e-5                # optimiser state, relative to max|ref|
CANARY = 1e30
PAD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def assert_close(a, b, rel, what=""):
    e = rel_err(a, b)
    print(f"{what}: rel err {e:.3e} (bound {rel:.3e})")
    assert e <= rel, f"{what}: rel err {e:.3e} > {rel:.3e}"


def assert_same(a, b, what=""):
    """Zero differing elements (NaNs in the same places count as equal)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = ~((a == b) | (torch.isnan(a) & torch.isnan(b))) if a.is_floating_point() else a != b
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ"


def grid_sizes():
    """n = 1, 3, 4; just over one workgroup's stride; every thread of the norm's fixed grid exactly one float4; that + 7 (a
    second trip and a 3-float tail)."""
    from weaklysuperviseddl_amd import ops
    full = ops.grad_norm_partials() * 256 * 4
    return [1, 3, 4, 256 * 4 + 4, full, full + 7], full


def canaried(values, dev):
    """Device buffer of len(values) + PAD floats, CANARY behind the values; returns (buffer, view of the values)."""
    buf = torch.full((values.numel() + PAD,), CANARY, dtype=torch.float32)
    buf[:values.numel()] = values
    buf = buf.to(dev)
    return buf, buf[:values.numel()]


def hyper(dev, lr=0.0, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, wd=0.0, mu=0.0, nesterov=False, max_norm=0.0, skip=False):
    return torch.tensor([lr, b1, b2, eps, grad_scale, wd, mu, float(nesterov), max_norm, float(skip)], dtype=torch.float32, device=dev)


def wide_values(n, seed):
    """N(0,1) times per-element scales from 1e-30 to 1e18 (fp32 values; their float64 norm is the reference)."""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 48.0 - 30.0)
    return (torch.randn(n, generator=g, dtype=torch.float64) * scale).float()


# ------------------------------------------------------------------------------------------------------------- 1. the norm
@gpu
def test_grad_norm_sizes_range_canaries_and_bits(dev):
    from weaklysuperviseddl_amd import ops
    sizes, full = grid_sizes()
    sizes.append(4 * full + 256 * 4 * 4 + 7)        # the four-loads-in-flight trip, a single-load trip for some threads, a tail
    gscale, max_norm = -0.37, 0.25                   # (|grad_scale| counts; the clip coefficient is checked on the way)
    for n in sizes:
        vals = wide_values(n, 100 + n % 97)
        buf, g = canaried(vals, dev)
        h = hyper(dev, grad_scale=gscale, max_norm=max_norm, skip=True)
        step_dev = torch.full((1,), 5, dtype=torch.int32, device=dev)
        stats = torch.zeros(ops.FLAT_STATS, device=dev)
        part = torch.full((ops.grad_norm_partials() + 8,), float("nan"), dtype=torch.float64, device=dev)
        ops.grad_norm(g, h, step_dev, stats, part)
        first = stats.clone()
        ops.grad_norm(g, h, step_dev, stats, part)
        assert_same(stats, first, f"norm n={n}: second call")
        want = O.total_norm(vals.numpy(), O.f32(gscale))
        got = stats.cpu().double().numpy()
        print(f"norm n={n}: got {got[0]:.9e} want {want:.9e}")
        assert abs(got[0] - want) <= ULP4 * want, (n, got[0], want)          # an over-read canary would add 1e60
        want_clip = O.clip_coef(want, max_norm)
        assert abs(got[1] - want_clip) <= ULP4 * want_clip, (n, got[1], want_clip)
        assert got[2] == 1.0 and got[3] == 0.0 and int(step_dev.item()) == 5
        assert torch.isnan(part[ops.grad_norm_partials():]).all()            # the partials stay inside their workspace
        assert_same(buf[n:], torch.full((PAD,), CANARY), f"norm n={n}: canaries")


@gpu
@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_grad_norm_nonfinite_skips(dev, poison):
    from weaklysuperviseddl_amd import ops
    _sizes, full = grid_sizes()
    n = full + 7
    vals = torch.randn(n, generator=torch.Generator().manual_seed(5))
    vals[n // 3] = poison
    _buf, g = canaried(vals, dev)
    step_dev = torch.full((1,), 5, dtype=torch.int32, device=dev)
    stats = torch.tensor([0., 1., 1., 2.], device=dev)
    ops.grad_norm(g, hyper(dev, max_norm=1.0, skip=True), step_dev, stats)
    got = stats.cpu()
    assert not torch.isfinite(got[0]) and got[2] == 0.0 and got[3] == 3.0 and int(step_dev.item()) == 4
    # without skip_nonfinite the step applies (and the counters stay), as clip_grad_norm_ + step() would
    ops.grad_norm(g, hyper(dev, max_norm=1.0, skip=False), step_dev, stats)
    got = stats.cpu()
    assert not torch.isfinite(got[0]) and got[2] == 1.0 and got[3] == 3.0 and int(step_dev.item()) == 4
    # in the tail (n & 3 floats, read by the first workgroup) as well
    vals[n // 3] = 0.0
    vals[n - 1] = poison
    ops.grad_norm(vals.to(dev), hyper(dev, skip=True), step_dev, stats)
    assert stats.cpu()[2] == 0.0 and int(step_dev.item()) == 3


@gpu
def test_grad_norm_above_float_max_counts_as_nonfinite(dev):
    """Four elements of 3e38: every square and the sum fit a double (norm 6e38), the float that is reported does not.  The
    contract judges the reported float: total_norm is inf and the step is skipped; the clip coefficient comes from the double."""
    from weaklysuperviseddl_amd import ops
    vals = torch.zeros(70)
    vals[[0, 17, 64, 69]] = torch.tensor([3e38, -3e38, 3e38, 3e38])
    want = O.total_norm(vals.numpy())
    assert np.isfinite(want) and want > float(np.finfo(np.float32).max)
    step_dev = torch.full((1,), 5, dtype=torch.int32, device=dev)
    stats = torch.tensor([0., 1., 1., 0.], device=dev)
    ops.grad_norm(vals.to(dev), hyper(dev, max_norm=1e10, skip=True), step_dev, stats)
    got = stats.cpu().double().numpy()
    assert np.isinf(got[0]) and got[2] == 0.0 and got[3] == 1.0 and int(step_dev.item()) == 4
    want_clip = O.f32(1e10) / want                  # 1.7e-29: a normal float
    assert abs(got[1] - want_clip) <= ULP4 * want_clip, (got[1], want_clip)
    orc = O.FlatOracle(O.SGD, np.ones(70), lr=0.1, max_norm=1.0, skip_nonfinite=True)
    assert orc.step(vals.numpy()) is False and orc.skipped == 1 and orc.step_no == 0


# ------------------------------------------------------------------------------------------------------------- 2. the step
ALGOS = {"sgd_nesterov": (O.SGD, 0.9, True), "sgd_momentum": (O.SGD, 0.9, False), "sgd_plain": (O.SGD, 0.0, False),
         "adam_l2": (O.ADAM_L2, 0.0, False), "adamw": (O.ADAMW, 0.0, False)}
STEP_GRID_CAP = 8192            # workgroups of the step kernel at most (as the Adam kernel's)


def run_flat_steps(dev, algo, mu, nesterov, wd, table, n, clip, seed):
    """3 steps of ops.flat_step on canaried buffers; returns the device buffers and the oracle."""
    from weaklysuperviseddl_amd import ops
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * s for s in (1.0, 0.1, 3.0)]
    lr, gscale = 1e-2, 0.5
    pb, p = canaried(p0, dev)
    mb, m = canaried(torch.zeros(n), dev)
    vb, v = canaried(torch.zeros(n), dev)
    if algo == O.SGD:
        v = None
        if mu == 0:
            m = None
    h = hyper(dev, lr=lr, grad_scale=gscale, wd=wd, mu=mu, nesterov=nesterov)
    stats = None if clip is None else torch.tensor([7.0, clip, 1.0, 0.0], device=dev)
    tab = None if table is None else torch.from_numpy(table).to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    orc = O.FlatOracle.as_kernel_reads(algo, p0.numpy(), lr=lr, weight_decay=wd, momentum=mu, nesterov=nesterov,
                       grad_scale=gscale * (1.0 if clip is None else clip), decay_blocks=table)
    for g in grads:
        _gb, gd = canaried(g, dev)
        ops.add_int(step_dev, 1)
        ops.flat_step(algo, p, gd, m, v, h, step_dev, stats, tab)
        orc.step(g.numpy())
    # apply == 0: one more launch that must change nothing
    if stats is not None:
        before = [pb.clone(), mb.clone(), vb.clone()]
        stats[2] = 0.0
        ops.flat_step(algo, p, gd, m, v, h, step_dev, stats, tab)
        for a, b, what in zip((pb, mb, vb), before, "pmv"):
            assert_same(a, b, f"apply = 0 left {what} alone")
    return (pb, mb, vb), orc


@gpu
@pytest.mark.parametrize("table_kind", ["null_table", "mixed_table"])
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["no_decay", "decay"])
@pytest.mark.parametrize("name", list(ALGOS))
def test_flat_step_against_the_oracle(dev, name, wd, table_kind):
    algo, mu, nesterov = ALGOS[name]
    sizes, full = grid_sizes()
    sizes = [3, 64, 64 * 5] + sizes[3:]
    if name in ("sgd_nesterov", "adamw") and wd and table_kind == "mixed_table":
        sizes.append(STEP_GRID_CAP * 256 * 4 + 7)     # past the step kernel's own grid cap: a second trip and a tail
    for k, n in enumerate(sizes):
        table = None
        if table_kind == "mixed_table":
            table = ((np.arange((n + 63) // 64) + k) % 3 == 0).astype(np.uint8)
        clip = 0.5 if table_kind == "mixed_table" else None          # stats_dev given / NULL
        (pb, mb, vb), orc = run_flat_steps(dev, algo, mu, nesterov, wd, table, n, clip, seed=n % 1000 + 3)
        what = f"{name} wd={wd} {table_kind} n={n}"
        assert_close(pb[:n], orc.p, STATE_TOL, what + " p")
        if not (algo == O.SGD and mu == 0):
            assert_close(mb[:n], orc.m, STATE_TOL, what + " m")
        else:
            assert_same(mb[:n], torch.zeros(n), what + " m untouched")
        if algo != O.SGD:
            assert_close(vb[:n], orc.v, STATE_TOL, what + " v")
        else:
            assert_same(vb[:n], torch.zeros(n), what + " v untouched")
        for b in (pb, mb, vb):
            assert_same(b[n:], torch.full((PAD,), CANARY), what + " canaries")
        (pb2, mb2, vb2), _ = run_flat_steps(dev, algo, mu, nesterov, wd, table, n, clip, seed=n % 1000 + 3)
        for a, b, w in zip((pb, mb, vb), (pb2, mb2, vb2), "pmv"):
            assert_same(a, b, what + f" second run {w}")


@gpu
def test_flat_step_refuses_bad_buffers(dev):
    from weaklysuperviseddl_amd import ops, WsdlError
    n = 64
    bufs = [torch.zeros(n + 4, device=dev) for _ in range(4)]
    h, step_dev = hyper(dev, lr=0.1), torch.ones(1, dtype=torch.int32, device=dev)
    good = [b[:n] for b in bufs]
    ops.flat_step(ops.FLAT_ADAMW, *good, h, step_dev)
    for i in range(4):                              # each buffer in turn 4 bytes off a 16-byte boundary
        args = list(good)
        args[i] = bufs[i][1:n + 1]
        with pytest.raises(WsdlError, match="16-byte aligned"):
            ops.flat_step(ops.FLAT_ADAMW, *args, h, step_dev)
    with pytest.raises(WsdlError):
        ops.flat_step(ops.FLAT_ADAM_L2, good[0], good[1], good[2], None, h, step_dev)       # Adam needs both moments
    with pytest.raises(WsdlError):
        ops.flat_step(7, *good, h, step_dev)
    with pytest.raises(WsdlError):
        ops.flat_step(ops.FLAT_SGD, *good, h[:5], step_dev)                                  # the five-float hyper_dev of Adam
    with pytest.raises(WsdlError):
        ops.flat_step(ops.FLAT_SGD, *good, h, step_dev, None, torch.ones(0, dtype=torch.uint8, device=dev))   # table too short
    with pytest.raises(WsdlError, match="16-byte aligned"):
        ops.grad_norm(bufs[0][1:n + 1], h, step_dev, torch.zeros(4, device=dev))
    ops.flat_step(ops.FLAT_SGD, good[0], good[1], None, None, h, None)                       # SGD without momentum: p and g only


# ------------------------------------------------------------------------------------------------------------- 3. defaults
SHAPES = [(5, 3), (70,), (64,), (2, 2, 2), (129,)]


def device_params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]


def flat_grads(opt, seed, scales):
    """Per step a gradient for the whole flat buffer, zero in the padding between parameters."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in scales:
        full = torch.zeros(opt.numel)
        for p, off in zip(opt.params, opt.offsets):
            full[off:off + p.numel()] = torch.randn(p.numel(), generator=g) * s
        out.append(full)
    return out


@gpu
def test_default_flat_adam_issues_the_old_launches(dev, monkeypatch):
    from weaklysuperviseddl_amd import ops, optim
    calls = []
    real_step, real_norm = ops.flat_step, ops.grad_norm
    monkeypatch.setattr(ops, "flat_step", lambda *a, **k: (calls.append("flat_step"), real_step(*a, **k))[1])
    monkeypatch.setattr(ops, "grad_norm", lambda *a, **k: (calls.append("grad_norm"), real_norm(*a, **k))[1])
    opt = optim.FlatAdam(device_params(dev, 1), 1e-2)
    pd, md, vd = opt.flat_param.clone(), torch.zeros_like(opt.flat_param), torch.zeros_like(opt.flat_param)
    h5 = torch.tensor([1e-2, 0.9, 0.999, 1e-8, 1.0], device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    for g in flat_grads(opt, 2, (1.0, 0.1, 3.0)):
        opt.zero_grad()
        opt.flat_grad.copy_(g)
        opt.step()
        ops.add_int(step_dev, 1)
        ops.adam_step_flat(pd, g.to(dev), md, vd, 0.0, 0.0, 0.0, 0.0, 0, step_dev=step_dev, hyper_dev=h5)
    assert calls == []
    assert_same(opt.flat_param, pd, "default FlatAdam p")
    assert_same(opt.exp_avg, md, "default FlatAdam exp_avg")
    assert_same(opt.exp_avg_sq, vd, "default FlatAdam exp_avg_sq")
    assert int(opt.step_dev.item()) == 3 and opt.step_count == 3
    # a five-parameter AdamW does go through the new entry points
    w = optim.FlatAdamW(device_params(dev, 1), 1e-2, max_grad_norm=1.0)
    w.zero_grad()
    w.flat_grad.copy_(g)
    w.step()
    assert calls == ["grad_norm", "flat_step"]


# ------------------------------------------------------------------------------------------------------------- 4. end to end
MAX_NORM = 1.0
SCALES = (3.0, 0.01, 2.0, 0.02)        # max_norm = 1: steps 1 and 3 clip, steps 2 and 4 do not


def make_flat(kind, params, no_decay, skip):
    from weaklysuperviseddl_amd import optim
    nd = [params[1], params[3]] if no_decay else None
    common = dict(max_grad_norm=MAX_NORM, skip_nonfinite=skip, no_decay=nd)
    if kind == "sgd":
        return optim.FlatSGD(params, 0.05, momentum=0.9, nesterov=True, weight_decay=1e-2, grad_scale=0.5, **common), \
            dict(algo=O.SGD, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2)
    if kind == "adamw":
        return optim.FlatAdamW(params, 0.05, grad_scale=0.5, **common), dict(algo=O.ADAMW, lr=0.05, weight_decay=1e-2)
    return optim.FlatAdam(params, 0.05, grad_scale=0.5, weight_decay=1e-2, **common), dict(algo=O.ADAM_L2, lr=0.05, weight_decay=1e-2)


@gpu
@pytest.mark.parametrize("segments", [False, True], ids=["one_launch", "segments"])
@pytest.mark.parametrize("kind", ["sgd", "adamw", "adam_l2"])
def test_optimisers_end_to_end_against_the_oracle(dev, kind, segments):
    """4 steps with clipping (whole buffer) - or, stepped in SEGMENTS with the table sliced on their boundaries, without it
    (clipping needs the whole norm and refuses segments)."""
    from weaklysuperviseddl_amd import optim
    params = device_params(dev, 4)
    opt, kw = make_flat(kind, params, True, False)
    if segments:
        opt.max_grad_norm = None
        opt.enable_early_step(first=64, growth=1, cap=64)
        assert len(opt.segments) == len(SHAPES)
        opt.early_step = True
    algo = kw.pop("algo")
    table = opt.decay_blocks.cpu().numpy()
    assert table.tolist() == [1, 0, 0, 1, 0, 1, 1, 1]
    orc = O.FlatOracle.as_kernel_reads(algo, opt.flat_param.cpu().numpy(), grad_scale=0.5, max_norm=opt.max_grad_norm, decay_blocks=table, **kw)
    clips = []
    for g in flat_grads(opt, 6, SCALES):
        opt.zero_grad()
        opt.flat_grad.copy_(g)
        opt.step()
        orc.step(g.numpy())
        what = f"{kind} step {orc.step_no}"
        assert_close(opt.flat_param, orc.p, STATE_TOL, what + " p")
        if opt.exp_avg is not None:
            assert_close(opt.exp_avg, orc.m, STATE_TOL, what + " m")
        if opt.exp_avg_sq is not None:
            assert_close(opt.exp_avg_sq, orc.v, STATE_TOL, what + " v")
        norm = float(opt.grad_norm())
        want = O.total_norm(g.numpy(), 0.5)             # (0.5 is a float32)
        assert abs(norm - want) <= ULP4 * want, (what, norm, want)
        clips.append(orc.clip < 1.0)
    if not segments:
        assert clips == [True, False, True, False]          # the oracle clipped on two steps and left two alone
    for p, off in zip(params, opt.offsets):                 # the parameters are still views of the flat buffer
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * off
    assert float(opt.skipped_steps()) == 0.0 and isinstance(opt, optim.FlatAdam)


@gpu
@pytest.mark.parametrize("kind", ["sgd", "adamw", "adam_l2"])
def test_nonfinite_gradient_is_skipped(dev, kind):
    """An inf planted in step 2: that step leaves every state tensor as it was, skipped_steps is 1, steps 3-4 equal the oracle
    that skipped (bias corrections of a run that never saw step 2)."""
    params = device_params(dev, 4)
    opt, kw = make_flat(kind, params, True, True)
    algo = kw.pop("algo")
    orc = O.FlatOracle.as_kernel_reads(algo, opt.flat_param.cpu().numpy(), grad_scale=0.5, max_norm=MAX_NORM, skip_nonfinite=True,
                       decay_blocks=opt.decay_blocks.cpu().numpy(), **kw)
    grads = flat_grads(opt, 8, SCALES)
    grads[1][opt.offsets[2] + 5] = float("inf")
    for i, g in enumerate(grads, 1):
        before = [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_dev) if t is not None]
        opt.zero_grad()
        opt.flat_grad.copy_(g)
        opt.step()
        applied = orc.step(g.numpy())
        assert applied == (i != 2)
        after = [t for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_dev) if t is not None]
        if i == 2:
            for a, b in zip(after, before):
                assert_same(a, b, f"{kind}: skipped step left state alone")
            assert not torch.isfinite(opt.grad_norm())
        else:
            assert_close(opt.flat_param, orc.p, STATE_TOL, f"{kind} step {i} p")
            if opt.exp_avg is not None:
                assert_close(opt.exp_avg, orc.m, STATE_TOL, f"{kind} step {i} m")
            if opt.exp_avg_sq is not None:
                assert_close(opt.exp_avg_sq, orc.v, STATE_TOL, f"{kind} step {i} v")
        assert float(opt.skipped_steps()) == (0.0 if i < 2 else 1.0)
    assert int(opt.step_dev.item()) == 3 == orc.step_no and opt.step_count == 4
    assert [t.data_ptr() for t in opt.state_tensors()][-1] == opt.stats_dev.data_ptr()      # what a launch plan restores


# ------------------------------------------------------------------------------------------------------------- 5. planned step
def _batch(B, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, S, S, generator=g)
    masks = (torch.rand(B, S, S, generator=g) > 0.5).long() * 255
    return img.to(dev), masks.to(dev)


def _segmentation_run(dev, planned, kind, kwargs, lr, steps, batches):
    from weaklysuperviseddl_amd import optim, plan
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    old = plan.PLAN_STEP[0]
    plan.PLAN_STEP[0] = planned
    try:
        torch.manual_seed(0)
        model = build_segmentation_model().to(dev).train()
        opt = make_optimizer(model, lr=lr, kind=kind, **kwargs)
        sched = optim.PolyLR(opt, total_steps=10)
        torch.manual_seed(1234)                     # identical dropout draws in both runs
        losses, plans, lrs, clips = [], [], [], []
        for i in range(steps):
            img, m = batches[i % len(batches)]
            losses.append(train_step(model, opt, img, m))
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            plans.append(None if st is None else st.plan)
            lrs.append(opt.lr)
            clips.append(opt.stats_dev[1].clone())
            sched.step()
        torch.cuda.synchronize()
        return model, opt, [float(l) for l in losses], st, plans, (lrs, [float(c) for c in clips])
    finally:
        plan.PLAN_STEP[0] = old


@pytest.fixture(scope="module")
def first_step_norm(dev):
    """Norm of the first eager step's gradient (the smallest model, batch and image size of tests/test_hip_plan.py), measured
    once: half of it is the clipping threshold of the planned-step tests, so clipping is active there."""
    batches = [_batch(4, 64, dev, 1)]
    _m, opt, _l, _st, _p, _lrs = _segmentation_run(dev, False, "sgd", dict(momentum=0.9), 1e-2, 1, batches)
    norm = float(opt.grad_norm())
    assert np.isfinite(norm) and norm > 0
    return norm


@gpu
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_planned_step_with_clipping_and_a_schedule(dev, kind, first_step_norm):
    """5 train_step calls with PolyLR between them: losses and all state bit-identical to the eager run; the plan recorded in
    call 3 is the one replayed in call 5 - the learning rate changes in device memory, not in the plan."""
    batches = [_batch(4, 64, dev, s) for s in (1, 2, 3)]
    M = 0.5 * first_step_norm
    kwargs = dict(momentum=0.9, weight_decay=1e-4, max_grad_norm=M) if kind == "sgd" else dict(max_grad_norm=M)
    lr = 1e-2 if kind == "sgd" else 1e-4
    m0, o0, l0, _, _, (lrs0, clips0) = _segmentation_run(dev, False, kind, kwargs, lr, 5, batches)
    m1, o1, l1, st, plans, (lrs1, clips1) = _segmentation_run(dev, True, kind, kwargs, lr, 5, batches)
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.records == 1 and st.replays == 2, (st.records, st.replays)
    assert plans[2] is not None and plans[4] is plans[2]
    assert lrs0 == lrs1 and len(set(lrs1)) == 5                     # a different rate in every call
    assert l0 == l1
    s0 = o0.state_tensors() + [b for b in m0.buffers()]
    s1 = o1.state_tensors() + [b for b in m1.buffers()]
    assert len(s0) == len(s1) and o0.stats_dev.data_ptr() in [t.data_ptr() for t in s0]
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
    stats = o1.stats_dev.cpu()
    assert float(o1.grad_norm()) > 0 and stats[2] == 1.0 and stats[3] == 0.0
    assert clips0 == clips1 and abs(clips1[0] - 0.5) < 1e-3          # clipping is active: M is half the first step's norm
    assert int(o1.step_dev.item()) == 5


# ------------------------------------------------------------------------------------------------------------- 6. early steps
@gpu
def test_clipping_refuses_early_segment_steps(dev):
    from weaklysuperviseddl_amd import nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    model = torch.nn.Sequential(wnn.Conv2d(3, 8, 3), wnn.Conv2d(8, 8, 3)).to(dev)
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(RuntimeError, match="optimizer.early_step = False"):
            make_optimizer(model, kind="sgd", momentum=0.9, early_step=True, **kw)
    opt = make_optimizer(model, kind="sgd", momentum=0.9, max_grad_norm=1.0, early_step=False)
    with pytest.raises(RuntimeError, match="optimizer.early_step = False"):
        opt.step_segment(0)
    make_optimizer(model, kind="sgd", momentum=0.9, weight_decay=1e-4, early_step=True)      # element-wise: segments are fine


@gpu
def test_graphed_step_refuses_the_new_launches_before_capture(dev):
    from weaklysuperviseddl_amd import nn as wnn
    from weaklysuperviseddl_amd.graph import GraphedTrainStep
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    model = torch.nn.Sequential(wnn.Conv2d(3, 8, 3)).to(dev)
    with pytest.raises(RuntimeError, match="train_step"):
        GraphedTrainStep(model, make_optimizer(model, kind="adamw"))
    GraphedTrainStep(model, make_optimizer(model))
