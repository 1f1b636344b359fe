"""The EMA teacher on the device (csrc/ema.hip, weaklysuperviseddl_amd/ema.py) against the float64 oracles of tests/ema_oracle.py.

The update kernels are held to the formula of include/wsdl_hip.h, ``float(fma(a, double(p) - double(e), double(e)))`` - the
oracle's emulated fused multiply-add: within one float32 ulp everywhere, at most 10 elements per million not bit-identical - and
to the unfused numpy evaluation within one ulp (on these inputs the two evaluations agree inside the same cap, because the decay
of an update is a float32 also during the warm-up: tests/test_ema.py::test_fused_and_unfused_oracle_agree_within_the_cap).
Through the optimiser: the launches
follow every step - eager, replayed from a launch plan, segment by segment - and a skipped step changes nothing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 10e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _words(dev, decay, warmup, k, apply=None):
    """hyper_ema_dev, step_dev, start_dev[, stats_dev] for the update number k (0-based)."""
    hyper = torch.tensor([decay, float(warmup)], device=dev, dtype=torch.float32)
    step = torch.tensor([k + 8], device=dev, dtype=torch.int32)
    start = torch.tensor([7], device=dev, dtype=torch.int32)
    stats = None if apply is None else torch.tensor([0.0, 1.0, float(apply), 0.0], device=dev, dtype=torch.float32)
    return hyper, step, start, stats


def _check_update(got, e, p, decay, warmup, k, what, unfused=True):
    want = O.ema_update_fma(e, p, decay, warmup, k).astype(np.float32)
    d = O.ulp_distance(got, want)
    assert d.max() <= 1, (what, int(d.max()))
    bad = int((d != 0).sum())
    assert bad <= CAP * got.size, (what, bad, got.size)
    if unfused:
        assert O.ulp_distance(got, O.ema_update32(e, p, decay, warmup, k)).max() <= 1, what
    return bad


# ------------------------------------------------------------------------------------------------------------- 1. flat kernel
@pytest.mark.parametrize("kind", O.DATA_KINDS)
@pytest.mark.parametrize("n", O.FLAT_SIZES)
def test_flat_ema_one_update(dev, n, kind):
    from weaklysuperviseddl_amd import ops
    e, p = O.flat_data(n, kind, 100 + n % 97)
    p_dev = torch.from_numpy(p).to(dev)
    for decay, warmup, k in O.flat_settings(n):
        e_dev = torch.from_numpy(e).to(dev)
        hyper, step, start, _ = _words(dev, decay, warmup, k)
        assert ops.flat_ema(e_dev, p_dev, hyper, step, start) is e_dev
        got = e_dev.cpu().numpy()
        if decay == 0.0:
            assert np.array_equal(got.view(np.uint32), p.view(np.uint32))      # a copy, also where |e| = 2^30 |p|
        else:
            _check_update(got, e, p, decay, warmup, k, (n, kind, decay, warmup, k))
    assert np.array_equal(p_dev.cpu().numpy(), p)   # p is untouched


@pytest.mark.parametrize("n", [1027, 4 * 256 * 3 + 2, 2 ** 23 + 1029])
def test_flat_ema_slices_repeats_and_skips(dev, n):
    """A call on [64, n) equals the same elements of the whole call; two calls are bit-identical; with apply = 0 every byte stays
    and the next applied update uses the same k."""
    from weaklysuperviseddl_amd import ops
    e, p = O.flat_data(n, "unit", 5)
    p_dev = torch.from_numpy(p).to(dev)
    hyper, step, start, stats = _words(dev, 0.999, True, 3, apply=1)
    runs = []
    for _ in range(2):
        e_dev = torch.from_numpy(e).to(dev)
        ops.flat_ema(e_dev, p_dev, hyper, step, start, stats)
        runs.append(e_dev)
    assert torch.equal(runs[0], runs[1])
    part = torch.from_numpy(e).to(dev)
    ops.flat_ema(part[64:], p_dev[64:], hyper, step, start, stats)
    assert torch.equal(part[64:], runs[0][64:]) and np.array_equal(part[:64].cpu().numpy(), e[:64])
    # skipped: the optimiser's finalize launch has taken the step number back and cleared apply
    skipped = torch.from_numpy(e).to(dev)
    stats[2] = 0.0
    ops.add_int(step, -1)
    ops.flat_ema(skipped, p_dev, hyper, step, start, stats)
    assert np.array_equal(skipped.cpu().numpy().view(np.uint32), e.view(np.uint32))
    stats[2] = 1.0
    ops.add_int(step, 1)
    ops.flat_ema(skipped, p_dev, hyper, step, start, stats)
    assert torch.equal(skipped, runs[0])


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_flat_ema_fifty_updates(dev, decay, warmup):
    """50 updates on drifting parameters: the device stays within max(4 x |float32 oracle - float64|, 2^-23 |value|) of the
    float64 trajectory (the standing bound of the state tests)."""
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    n = 4099
    rng = np.random.default_rng(9)
    e0 = rng.standard_normal(n).astype(np.float32)
    base, drift = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    e_dev = torch.from_numpy(e0).to(dev)
    p_dev = torch.empty(n, device=dev)
    hyper, step, start, _ = _words(dev, decay, warmup, -1)
    e64, e32, worst = e0.astype(np.float64), e0.copy(), 0.0
    for k in range(50):
        p = (base + np.float32(0.02 * k) * drift + rng.standard_normal(n).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        p_dev.copy_(torch.from_numpy(p))
        ops.add_int(step, 1)
        ops.flat_ema(e_dev, p_dev, hyper, step, start)
        e64 = O.ema_update(e64, p, decay, warmup, k)
        e32 = O.ema_update32(e32, p, decay, warmup, k)
        err = np.abs(e_dev.cpu().numpy().astype(np.float64) - e64)
        bound = np.maximum(4 * np.abs(e32.astype(np.float64) - e64), 2.0 ** -23 * np.abs(e64))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    report_line(f"flat_ema decay {decay} warmup {warmup}: 50 updates, worst device error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- 2. table kernel
TABLE_SIZES = (1, 3, 64, 2048, 5000, 4100)         # the last one 16-byte aligned: the float4 path, its tail, a second chunk trip


def _table_arena(dev, seed):
    """dst / src arenas with the tensors at odd float offsets (4-byte aligned, not 16) - the last at a multiple of 4 - and guard
    gaps in between."""
    rng = np.random.default_rng(seed)
    offs, n = [], 1
    for sz in TABLE_SIZES[:-1]:
        offs.append(n)
        n = (n + sz + 6) | 1            # a gap of at least six floats, the next start odd again
    n = (n + 3) // 4 * 4
    offs.append(n)
    n += TABLE_SIZES[-1]
    dst = rng.standard_normal(n + 8).astype(np.float32)
    src = rng.standard_normal(n + 8).astype(np.float32) + np.float32(0.5)
    return offs, dst, src


@pytest.mark.parametrize("mode", ["ema", "copy"])
def test_ema_table(dev, mode):
    from weaklysuperviseddl_amd import ops
    offs, dst, src = _table_arena(dev, 3)
    assert all(o % 4 for o in offs[:-1]) and offs[-1] % 4 == 0
    d_dev, s_dev = torch.from_numpy(dst).to(dev), torch.from_numpy(src).to(dev)
    assert d_dev.data_ptr() % 16 == 0 and s_dev.data_ptr() % 16 == 0
    pairs = [(d_dev[o:o + sz], s_dev[o:o + sz]) for o, sz in zip(offs, TABLE_SIZES)]
    table = ops.ema_table_entries(pairs, dev)
    decay, warmup, k = 0.999, True, 1
    hyper, step, start, stats = _words(dev, decay, warmup, k, apply=0)
    ops.ema_table(table, len(pairs), hyper, step, start, stats, mode)          # skipped: nothing moves
    assert np.array_equal(d_dev.cpu().numpy().view(np.uint32), dst.view(np.uint32))
    stats[2] = 1.0
    ops.ema_table(table, len(pairs), hyper, step, start, stats, mode)
    got = d_dev.cpu().numpy()
    touched = np.zeros(dst.size, bool)
    for o, sz in zip(offs, TABLE_SIZES):
        touched[o:o + sz] = True
        if mode == "copy":
            assert np.array_equal(got[o:o + sz], src[o:o + sz])
        else:
            _check_update(got[o:o + sz], dst[o:o + sz], src[o:o + sz], decay, warmup, k, ("table", sz))
    assert np.array_equal(got[~touched].view(np.uint32), dst[~touched].view(np.uint32))      # neighbouring memory
    assert np.array_equal(s_dev.cpu().numpy().view(np.uint32), src.view(np.uint32))
    again = torch.from_numpy(dst).to(dev)
    ops.ema_table(ops.ema_table_entries([(again[o:o + sz], s_dev[o:o + sz]) for o, sz in zip(offs, TABLE_SIZES)], dev), len(pairs),
                  hyper, step, start, None, mode)
    assert torch.equal(again, d_dev)


# ------------------------------------------------------------------------------------------------------------- 3. label correction
@pytest.mark.parametrize("content", O.TEACHER_CONTENTS)
@pytest.mark.parametrize("shape", O.TEACHER_SHAPES)
def test_teacher_targets(dev, shape, content):
    from weaklysuperviseddl_amd import ops
    logits, labels = O.teacher_case(shape, content, 11)
    lg, lab = torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev)
    out_buf, conf_buf = torch.empty_like(lab), torch.empty(lab.shape, device=dev)
    for tau in O.TEACHER_TAUS:
        tau_dev = torch.tensor([tau], device=dev, dtype=torch.float32)
        for mode in ("replace", "ignore"):
            want, wconf, wcounts, p64 = O.teacher_targets(logits, labels, tau, mode)
            near = (p64 > 0) & (np.abs(p64 - float(np.float32(tau))) <= O.TAU_BAND)
            assert near.sum() <= 1e-3 * near.size
            counts = torch.zeros(3, device=dev, dtype=torch.int64)
            got, conf = ops.teacher_targets(lg, lab, tau, mode, conf=True, counts=counts)
            what = (shape, content, tau, mode)
            assert O.ulp_distance(conf.cpu().numpy(), wconf).max() <= 1, what
            assert np.array_equal(got.cpu().numpy()[~near], want[~near]), what
            c = counts.cpu().numpy()
            assert c.sum() == labels.size and c[2] == wcounts[2] and np.abs(c - wcounts).max() <= near.sum(), (what, c, wcounts)
            if content == "agree":
                assert torch.equal(got, lab) and c[1] == 0
            if tau > 1:
                assert torch.equal(got, lab)
            # tau from device memory, out= reuse, accumulating counts, a second call
            r = ops.teacher_targets(lg, lab, tau_dev, mode, out=out_buf, conf=conf_buf, counts=counts)
            assert r[0] is out_buf and r[1] is conf_buf and torch.equal(out_buf, got) and torch.equal(conf_buf, conf)
            assert torch.equal(counts.cpu(), torch.from_numpy(2 * c))
            assert torch.equal(ops.teacher_targets(lg, lab, tau, mode), got)
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), logits.view(np.uint32)) and torch.equal(lab.cpu(), torch.from_numpy(labels))
    # strided logits: a channel slice of a wider tensor, and a permuted view
    B, C, H, W = shape
    wide = torch.randn(B, C + 3, H, W, device=dev)
    wide[:, 2:2 + C] = lg
    ref = ops.teacher_targets(lg, lab, 0.6, conf=True)
    for view in (wide[:, 2:2 + C], lg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
        r = ops.teacher_targets(view, lab, 0.6, conf=True)
        assert torch.equal(r[0], ref[0]) and torch.equal(r[1], ref[1])
    # dense logits whose base pointer is 4-byte but not 16-byte aligned: where H W % 4 == 0 this is the one-pixel-per-lane kernel
    # on a shape that otherwise takes four - both must give the bits that were checked against the oracle above
    arena = torch.empty(lg.numel() + 1, device=dev)
    off1 = arena[1:].view(shape)
    off1.copy_(lg)
    assert off1.is_contiguous() and off1.data_ptr() % 16 == 4 and lg.data_ptr() % 16 == 0
    counts = torch.zeros(3, device=dev, dtype=torch.int64)
    want_counts = torch.zeros(3, device=dev, dtype=torch.int64)
    ops.teacher_targets(lg, lab, 0.6, conf=True, counts=want_counts)
    r = ops.teacher_targets(off1, lab, 0.6, conf=True, counts=counts)
    assert torch.equal(r[0], ref[0]) and torch.equal(r[1], ref[1]) and torch.equal(counts, want_counts)


# ------------------------------------------------------------------------------------------------------------- 4. through the optimiser
def _batch(B, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, S, S, generator=g)
    masks = (torch.rand(B, S, S, generator=g) > 0.5).long() * 255
    return img.to(dev), masks.to(dev)


def _ulp_t(a, b):
    """float32 ulp distance on the device (finite values)."""
    def key(v):
        i = v.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (key(a) - key(b)).abs()


def _oracle_t(e_before, p, decay, warmup, k):
    """The fused oracle in float64 torch arithmetic on the device (tests/ema_oracle.py: only + - * of whole tensors)."""
    a = 1.0 - O.decay_at(decay, warmup, k)
    e64, p64 = e_before.double(), p.double()
    return p.clone() if a == 1.0 else O.fma_emulated(a, p64 - e64, e64).float()


def _assert_one_update(ema_now, ema_before, param_now, decay, warmup, k, what):
    d = _ulp_t(ema_now, _oracle_t(ema_before, param_now, decay, warmup, k))
    assert int(d.max()) <= 1, (what, int(d.max()))
    assert int((d != 0).sum()) <= CAP * d.numel(), (what, int((d != 0).sum()))


def _deeplab(dev, kind="adam", seed=0, ema_kwargs=None, attach=True, **opt_kwargs):
    from weaklysuperviseddl_amd import ema as E
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    torch.manual_seed(seed)
    model = build_segmentation_model().to(dev).train()
    opt = make_optimizer(model, lr=1e-4 if kind != "sgd" else 1e-2, kind=kind, **opt_kwargs)
    avg = E.FlatEMA(opt, model, build_segmentation_model().to(dev), **(ema_kwargs or {})) if attach else None
    return model, opt, avg


def _run(dev, planned, steps, batches, after_step=None, **kw):
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    old = plan.PLAN_STEP[0]
    plan.PLAN_STEP[0] = planned
    try:
        model, opt, avg = _deeplab(dev, **kw)
        torch.manual_seed(1234)                     # identical dropout draws in every run
        losses = []
        for i in range(steps):
            img, m = batches[i % len(batches)]
            before = None if after_step is None else (avg.ema_param.clone(), [tb.clone() for tb, _ in avg._float_bufs])
            losses.append(train_step(model, opt, img, m))
            if after_step is not None:
                after_step(i, model, opt, avg, before)
        torch.cuda.synchronize()
        st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
        return model, opt, avg, [float(l) for l in losses], st
    finally:
        plan.PLAN_STEP[0] = old


def _follows_oracle(decay=0.999, warmup=True, buffers="ema"):
    def check(i, model, opt, avg, before):
        e0, b0 = before
        _assert_one_update(avg.ema_param, e0, opt.flat_param, decay, warmup, i, f"step {i + 1}: ema_param")
        for (tb, sb), old in zip(avg._float_bufs, b0):
            if buffers == "copy":
                assert torch.equal(tb, sb)
            else:
                _assert_one_update(tb, old, sb, decay, warmup, i, f"step {i + 1}: buffer")
        assert int(avg.updates()) == i + 1
    return check


@pytest.fixture(scope="module")
def eager_and_planned(dev):
    batches = [_batch(2, 64, dev, s) for s in (1, 2, 3)]
    seen = []
    eager = _run(dev, False, 6, batches, after_step=_follows_oracle())
    planned = _run(dev, True, 6, batches, after_step=lambda i, m, o, avg, b: seen.append(avg.ema_param.clone()))
    return eager, planned, seen


def test_planned_run_with_an_ema_is_bit_identical_to_the_eager_run(dev, eager_and_planned):
    """Six train_step calls: parameters, the average and the teacher's buffers equal the eager run's bit for bit; the steps that
    were replayed moved the average - the plan holds the EMA launches.  (The eager run checked every update against the oracle
    applied to the device's own parameter sequence.)"""
    (m0, o0, a0, l0, _), (m1, o1, a1, l1, st), seen = eager_and_planned
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.records == 1 and st.replays == 3, (st.records, st.replays)
    assert l0 == l1
    assert torch.equal(o0.flat_param, o1.flat_param) and torch.equal(a0.ema_param, a1.ema_param)
    assert len(a0._float_bufs) > 100
    for (t0, _), (t1, _) in zip(a0._float_bufs, a1._float_bufs):
        assert torch.equal(t0, t1)
    for a, b in zip(o0.state_tensors(), o1.state_tensors()):
        assert torch.equal(a, b)
    assert not torch.equal(seen[4], seen[3]) and not torch.equal(seen[5], seen[4])          # replayed steps 5 and 6
    assert int(a1.updates()) == 6 and a1.ema_param.data_ptr() in [t.data_ptr() for t in o1.state_tensors()]
    # the teacher's parameters are views of the average at the student's offsets and carry no gradient
    tp = dict(a1.teacher.named_parameters())
    for (name, sp), off in zip(((n, p) for n, p in m1.named_parameters() if p.requires_grad), o1.offsets):
        assert tp[name].data_ptr() == a1.ema_param.data_ptr() + 4 * off and not tp[name].requires_grad
    assert not a1.teacher.training


@pytest.fixture(scope="module")
def default_planned(dev):
    """Four planned train_step calls WITHOUT an EMA at B = 2, 64 x 64: the default path."""
    batches = [_batch(2, 64, dev, s) for s in (1, 2, 3)]
    return _run(dev, True, 4, batches, attach=False)


def test_default_path_issues_the_launches_it_always_issued(dev, eager_and_planned, default_planned):
    """Without an EMA the optimiser reports the three-element key and the recorded step holds exactly the EMA's two launches
    fewer (the flat average and the buffer table)."""
    (_m, _o, _a, _l, _), (_m1, o1, _a1, _l1, st_ema), _seen = eager_and_planned
    _m2, o2, avg, _l2, st = default_planned
    assert avg is None and o2.ema is None and o2.launch_key() == (None, False, False) and len(o1.launch_key()) == 4
    assert st.disabled is None and st.replays == 1
    assert st.plan.stats["kernels"] + 2 == st_ema.plan.stats["kernels"]
    assert [t.data_ptr() for t in o2.state_tensors()] == [t.data_ptr() for t in (o2.flat_param, o2.exp_avg, o2.exp_avg_sq, o2.step_dev,
                                                                                 o2.stats_dev)]


@pytest.mark.parametrize("kind,kwargs,ema_kwargs", [("sgd", dict(momentum=0.9), dict(decay=0.9, warmup=False, buffers="copy")),
                                                    ("adamw", {}, dict(decay=0.99))])
def test_other_optimisers_drive_the_same_average(dev, kind, kwargs, ema_kwargs):
    batches = [_batch(2, 64, dev, s) for s in (1, 2)]
    check = _follows_oracle(ema_kwargs["decay"], ema_kwargs.get("warmup", True), ema_kwargs.get("buffers", "ema"))
    _run(dev, False, 2, batches, after_step=check, kind=kind, ema_kwargs=ema_kwargs, **kwargs)


def test_early_segment_steps_give_the_same_average(dev):
    batches = [_batch(2, 64, dev, s) for s in (1, 2, 3)]
    _m0, o0, a0, l0, _ = _run(dev, False, 3, batches)
    _m1, o1, a1, l1, _ = _run(dev, False, 3, batches, early_step=True)
    assert o1.early_step and len(o1.segments) > 1 and o0.early_step is False
    assert l0 == l1 and torch.equal(o0.flat_param, o1.flat_param)
    assert torch.equal(a0.ema_param, a1.ema_param)
    for (t0, _), (t1, _) in zip(a0._float_bufs, a1._float_bufs):
        assert torch.equal(t0, t1)


def test_teacher_caches_never_go_stale(dev):
    """After step 1 and again after step 2 the teacher's eval-mode prediction equals, bit for bit, a freshly built model that
    loaded the teacher's state dict; the two predictions differ."""
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    x = _batch(2, 64, dev, 9)[0]
    preds = []

    def look(i, model, opt, avg, before):
        with torch.no_grad():
            got = avg.teacher(x)["out"].clone()
            fresh = build_segmentation_model().to(dev).eval()
            fresh.load_state_dict(avg.teacher.state_dict())
            assert torch.equal(got, fresh(x)["out"]), f"after step {i + 1}"
        preds.append(got)
    _run(dev, False, 2, [_batch(2, 64, dev, s) for s in (1, 2)], after_step=look, ema_kwargs=dict(decay=0.5, warmup=False))
    assert not torch.equal(preds[0], preds[1])


# ---- on a small network with hand-made gradients -------------------------------------------------------------------------------
def _small(dev, seed=0, **opt_kwargs):
    from weaklysuperviseddl_amd import ema as E, nn as wnn, optim
    torch.manual_seed(seed)

    def net():
        return torch.nn.Sequential(wnn.Conv2d(3, 8, 3, padding=1, bias=False), wnn.BatchNorm2d(8), wnn.Conv2d(8, 5, 1, bias=True)).to(dev)
    model = net()
    opt = optim.FlatAdam(model.parameters(), lr=1e-2, **opt_kwargs)
    return model, opt, net, E


def _grad(opt, seed):
    return torch.randn(opt.numel, generator=torch.Generator().manual_seed(seed)).to(opt.flat_param.device)


def _manual_step(opt, g):
    opt.zero_grad()
    opt.flat_grad.copy_(g)
    opt.step()


def test_a_skipped_step_leaves_the_average_alone(dev):
    model, opt, net, E = _small(dev, skip_nonfinite=True)
    avg = E.FlatEMA(opt, model, net(), decay=0.999)
    _manual_step(opt, _grad(opt, 1))
    e1, b1 = avg.ema_param.clone(), [tb.clone() for tb, _ in avg._float_bufs]
    bad = _grad(opt, 2)
    bad[opt.offsets[1] + 3] = float("inf")
    model[1].running_mean.add_(1.0)                 # the student's statistics move on whether or not the step is applied
    _manual_step(opt, bad)
    assert float(opt.skipped_steps()) == 1.0 and int(avg.updates()) == 1
    assert torch.equal(avg.ema_param.view(torch.int32), e1.view(torch.int32))
    for (tb, _), old in zip(avg._float_bufs, b1):
        assert torch.equal(tb, old)
    _manual_step(opt, _grad(opt, 3))                # the next applied update is number 1 (0-based), not 2
    assert int(avg.updates()) == 2
    _assert_one_update(avg.ema_param, e1, opt.flat_param, 0.999, True, 1, "after the skip")
    assert not torch.equal(_oracle_t(e1, opt.flat_param, 0.999, True, 2), _oracle_t(e1, opt.flat_param, 0.999, True, 1))


def test_state_dict_round_trip(dev):
    model, opt, net, E = _small(dev)
    avg = E.FlatEMA(opt, model, net(), decay=0.99)
    for s in (1, 2):
        _manual_step(opt, _grad(opt, s))
    state = avg.state_dict()
    assert state["updates"] == 2 and state["decay"] == 0.99 and state["warmup"] is True
    saved = [t.clone() for t in opt.state_tensors()]
    _manual_step(opt, _grad(opt, 3))
    # (the teacher's parameters, not the whole buffer: a state dict does not carry the padding between them, which the
    # hand-made gradients of this test move as well)
    want, want_bufs = [p.clone() for p in avg.teacher.parameters()], [tb.clone() for tb, _ in avg._float_bufs]
    for t, s in zip(opt.state_tensors(), saved):    # back to the state the dict was taken at, with a NEW average
        t.copy_(s)
    opt.step_count = 2
    opt.ema = None
    again = E.FlatEMA(opt, model, net(), decay=0.5, warmup=False)
    with pytest.raises(ValueError, match="buffers='copy'"):
        again.load_state_dict(dict(state, buffers="copy"))
    again.load_state_dict(state)
    assert int(again.updates()) == 2 and again.decay == 0.99 and again.warmup is True
    _manual_step(opt, _grad(opt, 3))
    assert all(torch.equal(p, w) for p, w in zip(again.teacher.parameters(), want)) and int(again.updates()) == 3
    for (tb, _), w in zip(again._float_bufs, want_bufs):
        assert torch.equal(tb, w)
    # reset: teacher <- student, the warm-up starts over; set_decay reaches the device
    again.reset()
    assert torch.equal(again.ema_param, opt.flat_param) and int(again.updates()) == 0
    again.set_decay(0.25)
    assert again.hyper_dev.tolist() == [0.25, 1.0]


def test_graphed_step_refuses_an_attached_ema(dev):
    from weaklysuperviseddl_amd.graph import GraphedTrainStep
    model, opt, net, E = _small(dev)
    GraphedTrainStep(model, opt)
    E.FlatEMA(opt, model, net())
    with pytest.raises(RuntimeError, match="EMA"):
        GraphedTrainStep(model, opt)


# ------------------------------------------------------------------------------------------------------------- 5. callers
def _dataset(dev, n=4, S=64, seed=4):
    from weaklysuperviseddl_amd.TraditionalModel import InMemoryPseudoDataset
    g = torch.Generator().manual_seed(seed)
    return InMemoryPseudoDataset(torch.randn(n, 3, S, S, generator=g).to(dev), ((torch.rand(n, S, S, generator=g) > 0.5) * 255).to(dev))


def _compose(teacher, images, masks, **kw):
    from weaklysuperviseddl_amd import ops
    teacher.eval()
    with torch.no_grad():
        logits = teacher(images)["out"]
    return ops.teacher_targets(logits, ops.clamp_max_labels(masks.long(), 1), **kw)


def test_refine_dataset_with_the_teacher_method(dev):
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss import refine_dataset
    torch.manual_seed(0)
    model = build_segmentation_model().to(dev).eval()
    data = _dataset(dev)
    before = data.masks.clone()
    want = _compose(model, data.images, before, tau=0.5)          # (two classes: the maximum is at least 0.5 - every pixel is confident)
    refine_dataset(model, data, chunk=3, method="teacher", teacher_kwargs={"tau": 0.5})
    assert torch.equal(data.masks, (want > 0).to(torch.uint8) * 255) and set(data.masks.unique().tolist()) <= {0, 255}
    assert not torch.equal(data.masks, before) and int(want.min()) >= 0          # something was corrected; -100 never reaches the masks
    with pytest.raises(ValueError, match="'ignore' mode"):
        refine_dataset(model, data, method="teacher", teacher_kwargs={"mode": "ignore"})


def test_alternation_hands_the_teacher_to_evaluate_and_refinement(dev):
    from weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss import run_alternating_training
    model, opt, avg = _deeplab(dev, ema_kwargs=dict(decay=0.5))
    data = _dataset(dev)
    before = data.masks.clone()
    got = []
    run_alternating_training(model, opt, data, num_alternations=1, epochs_per_round=1, first_batch_size=2, refine_chunk=4,
                             refine_kwargs={"method": "teacher", "teacher_kwargs": {"tau": 0.5}}, evaluate=lambda m: got.append(m) or {},
                             device=dev, log=None, ema=avg)
    assert len(got) == 1 and got[0] is avg.teacher and got[0] is not model
    assert int(avg.updates()) == 2
    want = _compose(avg.teacher, data.images, before, tau=0.5)
    assert torch.equal(data.masks, (want > 0).to(torch.uint8) * 255)
    with pytest.raises(ValueError, match="FlatEMA of this model"):
        run_alternating_training(_deeplab(dev, attach=False)[0], opt, data, num_alternations=1, ema=avg, log=None)


def test_mean_teacher_step_equals_its_composition_and_replays_the_plan(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import train_step, train_step_mean_teacher
    batches = [_batch(2, 64, dev, s) for s in (1, 2, 3)]

    def run(composed):
        model, opt, avg = _deeplab(dev, ema_kwargs=dict(decay=0.5, warmup=False))
        torch.manual_seed(1234)
        losses, ignored = [], 0
        for i in range(4):
            img, m = batches[i % 3]
            if composed:
                with torch.no_grad():
                    logits = avg.teacher(img)["out"]
                labels = ops.teacher_targets(logits, ops.clamp_max_labels(m.long(), 1), 0.5, "ignore")
                ignored += int((labels == -100).sum())
                losses.append(float(train_step(model, opt, img, labels)))
            else:
                losses.append(float(train_step_mean_teacher(model, avg, opt, img, m, tau=0.5)))
            st = next(iter(opt.__dict__["_wsdl_planned"].values()))
            if i == 2:
                assert st.records == 1 and st.disabled is None, st.disabled         # the third call records and verifies ...
        assert st.replays == 1 and st.disabled is None, st.disabled                 # ... the fourth replays
        return opt, avg, losses, ignored
    o0, a0, l0, ignored = run(True)
    o1, a1, l1, _ = run(False)
    assert ignored > 0                                                             # the teacher did mark pixels: -100 went through the plan
    assert l0 == l1 and torch.equal(o0.flat_param, o1.flat_param) and torch.equal(a0.ema_param, a1.ema_param)


def _optimizer_of(model):
    return next(model.parameters())._wsdl_grad_sink            # the flat optimiser that owns the parameters


def test_train_segmentation_model_with_and_without_an_ema(dev, tmp_path):
    """``train_segmentation_model`` on a tiny pseudo-mask run (five 64 x 64 PNG pairs, batches of 2, two epochs = four steps).
    Without ``ema=``: no average is attached, the optimiser's key is the default triple, and the run equals - recorded kernel
    count, loss and every parameter bit - the function's body as it was before it knew of an EMA, written out by hand below
    (model, optimiser, loader, per epoch the steps and the validation).  With ``ema={...}``: a teacher of the model's own head is built and left
    as ``model.ema``, it has taken one update per step, its plan holds the two EMA kernels more, and it is validated beside
    the student every epoch."""
    from PIL import Image
    from weaklysuperviseddl_amd import ema as E
    from weaklysuperviseddl_amd.TraditionalModel import SegmentationModel, train_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.PsuedoMasks import _to_png_u8
    rng = np.random.RandomState(4)
    for d in ("images_t1", "pseudo_masks_t1"):
        (tmp_path / d).mkdir()
    for i in range(5):                                   # batch_size 2 -> batches of 2, 2, 1 (the last one skipped)
        m = np.zeros((64, 64), np.uint8)
        m[10 + 4 * i:50, 8:40 + 3 * i] = 1
        Image.fromarray(_to_png_u8(torch.from_numpy(m).float().unsqueeze(0).expand(3, -1, -1))).save(tmp_path / "pseudo_masks_t1" / f"{i}.png")
        Image.fromarray(_to_png_u8(torch.from_numpy(rng.rand(3, 64, 64).astype(np.float32)))).save(tmp_path / "images_t1" / f"{i}.png")
    val = [(torch.rand(1, 3, 64, 64), (torch.tensor([0]), torch.randint(1, 4, (1, 64, 64))))]

    def planned(opt):
        return next(iter(opt.__dict__["_wsdl_planned"].values()))

    def by_hand():
        from torch.utils.data import DataLoader
        from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, evaluate_model, train_step
        from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import PseudoSegmentationDataset
        from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
        torch.manual_seed(0)
        data = PseudoSegmentationDataset(img_dir=str(tmp_path / "images_t1"), mask_dir=str(tmp_path / "pseudo_masks_t1"), transform=True)
        loader = DataLoader(data, batch_size=2, shuffle=True, num_workers=0, generator=torch.Generator().manual_seed(3))
        model = build_segmentation_model(num_classes=2).to(dev)
        opt = make_optimizer(model, lr=1e-4)
        for _epoch in range(2):
            model.train()
            total = torch.zeros((), device=dev)
            for images, masks in loader:
                if images.size(0) == 1:
                    continue
                total += train_step(model, opt, images.to(dev), masks.to(dev), loss_fn="cross_entropy", criterion=None)
            final = total.item()
            evaluate_model(model, val, device=dev, binarize="modular")
        return opt, final
    hand_opt, hand_loss = by_hand()
    default_kernels = planned(hand_opt).plan.stats["kernels"]

    def run(**kw):
        logs = []
        torch.manual_seed(0)
        model, final_loss = train_segmentation_model("cross_entropy", "t1", 1e-4, 2, 2, 0.2, out_root=str(tmp_path), device=dev,
                                                     val_loader=val, seed=3, log=logs.append, **kw)
        opt = _optimizer_of(model)
        st = planned(opt)
        assert np.isfinite(final_loss) and opt.step_count == 4 and int(opt.step_dev) == 4
        assert st.disabled is None and st.records == 1 and st.replays == 1, st.disabled
        return model, opt, st, logs, final_loss

    model, opt, st, logs, loss = run()
    assert opt.ema is None and not hasattr(model, "ema") and opt.launch_key() == (None, False, False)
    assert st.plan.stats == planned(hand_opt).plan.stats and loss == hand_loss
    assert torch.equal(opt.flat_param, hand_opt.flat_param) and torch.equal(opt.exp_avg_sq, hand_opt.exp_avg_sq)
    assert sum("Validation IoU" in x for x in logs) == 2 and not any("EMA teacher" in x for x in logs)

    model, opt, st, logs, _loss = run(ema={"decay": 0.9, "warmup": False})
    avg = model.ema
    assert isinstance(avg, E.FlatEMA) and opt.ema is avg and avg.decay == 0.9 and avg.warmup is False
    assert isinstance(avg.teacher, SegmentationModel) and avg.teacher is not model and not avg.teacher.training
    assert avg.teacher.classifier[-1].out_channels == 2 and avg.teacher.aux_classifier is not None
    assert "ema" not in dict(model.named_modules()) and not any(k.startswith("ema") for k in model.state_dict())
    assert int(avg.updates()) == 4 and len(opt.launch_key()) == 4
    assert st.plan.stats["kernels"] == default_kernels + 2
    assert sum("EMA teacher validation IoU" in x for x in logs) == 2 and sum("Validation IoU" in x for x in logs) == 2
    assert not torch.equal(avg.ema_param, opt.flat_param)


def test_mean_teacher_step_weighted_by_confidence_replays_the_plan(dev):
    """``weight_by_conf=True``: the teacher's confidence becomes the criterion's pixel weight - a buffer with a stable address
    - and the student's step with that criterion is recorded in the third call and replayed in the fourth, equal to the same
    four calls issued eagerly."""
    from weaklysuperviseddl_amd import nn as wnn, ops, plan
    from weaklysuperviseddl_amd.TraditionalModel import train_step_mean_teacher
    batches = [_batch(2, 64, dev, s) for s in (1, 2, 3)]

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            model, opt, avg = _deeplab(dev, ema_kwargs=dict(decay=0.5, warmup=False))
            crit = wnn.CrossEntropyLoss()
            torch.manual_seed(1234)
            losses = []
            for i in range(4):
                img, m = batches[i % 3]
                losses.append(float(train_step_mean_teacher(model, avg, opt, img, m, crit, tau=0.5, mode="replace", weight_by_conf=True)))
            with torch.no_grad():
                logits = avg.teacher(img)["out"]
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            return opt, avg, crit, losses, st, logits
        finally:
            plan.PLAN_STEP[0] = old
    o0, a0, _c0, l0, _st0, _ = run(False)
    o1, a1, crit, l1, st, _ = run(True)
    assert st is not None and st.disabled is None and st.records == 1 and st.replays == 1, getattr(st, "disabled", None)
    assert all(np.isfinite(l1)) and l0 == l1
    assert torch.equal(o0.flat_param, o1.flat_param) and torch.equal(a0.ema_param, a1.ema_param)
    w = crit.pixel_weight
    assert tuple(w.shape) == (2, 64, 64) and float(w.min()) >= 0.5 and float(w.max()) <= 1.0
