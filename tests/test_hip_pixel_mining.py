"""Pixel mining on the device: the segmented radix select (``ops.kth_value``) against an exact host selection, and
``ops.cross_entropy_mined`` / ``wnn.MinedCrossEntropyLoss`` against the existing cross-entropy kernel (bit for bit), the float64
oracle (tests/pixel_mining_oracle.py), their tie and edge rules, planned training steps and the untouched default path."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_mining_oracle import boundary_gaps, kth_value_exact, mined_ce  # noqa: E402

# Every test that takes the `dev` fixture MUST carry @gpu (see test_hip_small_ops.py)
gpu = pytest.mark.gpu

# the bound tests/test_hip_weighted_ce.py holds the cross-entropy kernel to - the same kernel produces the mined loss
REL = 1e-5
# a selection may only be compared when no pixel can change sides through float32 rounding of its loss: the float64 distances
# that decide it must be ten times the bound
GAP = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def make_case(shape, seed, ignore_index=-100, scale=3.0):
    """As make_case of tests/test_hip_weighted_ce.py."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g) * scale
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.2] = ignore_index
    w = torch.rand(C, generator=g) + 0.25
    p = torch.rand(B, H, W, generator=g) + 0.05
    return z, y, w, p


def run_mined(dev, z, y, weight=None, eps=0.0, pw=None, reduction="mean", upstream=0.7, **sel):
    from weaklysuperviseddl_amd import ops
    zd = z.to(dev).requires_grad_(True)
    stats = {}
    loss = ops.cross_entropy_mined(zd, y.to(dev), -100, weight=None if weight is None else weight.to(dev), label_smoothing=eps,
                                   pixel_weight=None if pw is None else pw.to(dev), reduction=reduction, stats=stats, **sel)
    loss.backward(torch.tensor(upstream, device=dev))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert stats["threshold"].dtype == torch.float32 and stats["kept"].dtype == torch.int64 and stats["valid"].dtype == torch.int64
    return loss.detach().cpu(), zd.grad.cpu(), {k: v.cpu() for k, v in stats.items()}


# ------------------------------------------------------------------------------------------------ 1. the select is exact
STRIDE = 256 * 256          # elements one pass of the capped grid covers (256 workgroups of 256 threads): above it they loop
SIZES = (1, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, 200003)


def _bits(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def _data(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 1.25, np.float32)
    if kind == "two_values":
        return rng.choice(np.array([0.5, 2.0], np.float32), n)
    if kind == "low_byte":
        return _bits(0x3F800000 | rng.integers(0, 256, n, dtype=np.uint32))
    if kind == "high_byte":         # bit 23 of the constant part is 0: the exponent never reaches 255, every value is finite
        return _bits((rng.integers(0, 256, n, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00345678))
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "mixed":
        special = np.array([0.0, -0.0, 1e-40, -1e-41, 1.4e-45, np.inf, -np.inf, 3.4e38, -3.4e38], np.float32)
        pick = rng.random(n) < 0.3
        x[pick] = rng.choice(special, int(pick.sum()))
        return x
    if kind == "nans":
        x[rng.random(n) < 0.1] = np.nan
        if n == 1:
            x[0] = np.nan
        return x
    raise ValueError(kind)


KINDS = ("normal", "equal", "two_values", "low_byte", "high_byte", "mixed", "nans")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_kth_value_is_exact(dev, kind):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(KINDS.index(kind))
    for n in SIZES:
        x = _data(kind, n, rng)
        xd = torch.from_numpy(x).to(dev)
        nc = int((~np.isnan(x)).sum())
        ranks = [(1, 0.0), (nc, 0.0), (nc + 5, 0.0), (0, 0.0), (1, 0.25), (1, 0.5)]
        got = []
        for (k, frac), largest in itertools.product(ranks, (True, False)):
            a = ops.kth_value(xd, k, frac, largest=largest)
            b = ops.kth_value(xd, k, frac, largest=largest)
            got.append((k, frac, largest, a, b))
        for k, frac, largest, (v, cnt), (v2, cnt2) in got:        # (read back after everything was enqueued)
            want, want_n = kth_value_exact(x, k, frac, largest)
            what = (kind, n, k, frac, largest)
            assert tuple(v.shape) == (1,) and v.dtype == torch.float32 and cnt.dtype == torch.int64, what
            assert v.item() == float(want) and cnt.item() == want_n, (what, v.item(), float(want), cnt.item(), want_n)
            assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(cnt, cnt2), what      # two runs: the same bits


@gpu
@pytest.mark.parametrize("n", (257, STRIDE // 3 + 1, 70001))     # segments = 3: 85 workgroups each - no loop, just a loop, loops
def test_kth_value_segments_and_valid_masks(dev, n):
    from weaklysuperviseddl_amd import ops
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)).astype(np.float32)
    x[0, ::11] = np.nan
    valid = np.zeros((3, n), np.uint8)
    valid[0] = rng.random(n) < 0.5
    valid[2] = 1                                    # segment 1: no candidate at all
    xd, vd = torch.from_numpy(x).to(dev), torch.from_numpy(valid).to(dev)
    for (k, frac), largest, mask in itertools.product(((1, 0.0), (0, 0.0), (5, 0.25), (1, 0.5), (n, 0.0), (0, 1.0)), (True, False),
                                                      ("uint8", "bool", None)):
        m = None if mask is None else (vd if mask == "uint8" else vd.bool())
        v, cnt = ops.kth_value(xd, k, frac, largest=largest, valid=m, segments=3)
        v, cnt = v.cpu().numpy(), cnt.cpu().numpy()
        for s in range(3):
            want, want_n = kth_value_exact(x[s], k, frac, largest, None if mask is None else valid[s])
            assert v[s] == want and cnt[s] == want_n, (n, k, frac, largest, mask, s, v[s], want, cnt[s], want_n)
    # a non-contiguous view is selected over as the dense tensor it stands for
    v, cnt = ops.kth_value(xd.t()[:, :2], 3, largest=True)
    want, want_n = kth_value_exact(np.ascontiguousarray(x.T[:, :2]), 3, 0.0, True)
    assert v.item() == want and cnt.item() == want_n
    # arguments the ABI refuses
    from weaklysuperviseddl_amd._lib import lib
    val, cn = torch.empty(3, device=dev), torch.empty(3, dtype=torch.int64, device=dev)
    ws = ops.workspace(lib().wsdl_kth_workspace(3), dev)
    ok = (xd.data_ptr(), None, n, 3, 1, 1, 0.5, val.data_ptr(), cn.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    assert lib().wsdl_kth_value(*ok) == 0
    for i, bad in ((2, 0), (2, 1 << 31), (3, 0), (5, -1), (6, 1.5), (6, -0.1), (6, float("nan")), (10, 16), (9, ws.data_ptr() + 1)):
        args = list(ok)
        args[i] = bad
        assert lib().wsdl_kth_value(*args) != 0, (i, bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. identity with the existing kernel, bit for bit
@gpu
@pytest.mark.parametrize("full", (False, True))
def test_mined_loss_is_the_existing_kernel_with_the_published_selection(dev, full):
    from weaklysuperviseddl_amd import ops
    B, C, H, W = 3, 3, 33, 40
    z, y, w, p = make_case((B, C, H, W), 21)
    p[p < 0.25] = 0.0                                               # a pixel weight with zeros: no candidates
    weight, eps, pw = (w, 0.1, p) if full else (None, 0.0, None)
    variants = [dict(mode="hard", thresh=0.7, min_kept=100), dict(mode="hard", thresh=None, min_kept=50),
                dict(mode="hard", thresh=0.2, min_kept=0), dict(mode="trim", drop_frac=0.25), dict(mode="trim", drop_frac=0.0)]
    nll = ops.cross_entropy(z.to(dev), y.to(dev), -100, reduction="none").cpu()
    valid = (y != -100) & ((pw if pw is not None else torch.ones(B, H, W)) != 0)
    for sel, scope, reduction in itertools.product(variants, ("batch", "image"), ("mean", "sum")):
        loss, grad, st = run_mined(dev, z, y, weight, eps, pw, reduction, scope=scope, **sel)
        S = B if scope == "image" else 1
        thr = st["threshold"].reshape(S, 1)
        if sel["mode"] == "hard":
            cap = float("inf") if sel["thresh"] is None else float(np.float32(-np.log(np.float64(sel["thresh"]))))
            chosen = nll.reshape(S, -1) >= torch.clamp(thr, max=cap)
        else:
            chosen = nll.reshape(S, -1) <= thr
        chosen = chosen & valid.reshape(S, -1)
        m = chosen.reshape(B, H, W).float() * (pw if pw is not None else 1.0)
        what = (sel, scope, reduction, full)
        assert torch.equal(st["selection"], m), what
        assert torch.equal(st["kept"], chosen.sum(1)) and torch.equal(st["kept"], m.reshape(S, -1).count_nonzero(1)), what
        assert torch.equal(st["valid"], valid.reshape(S, -1).sum(1)), what
        zd = z.to(dev).requires_grad_(True)
        ref = ops.cross_entropy(zd, y.to(dev), -100, weight=None if weight is None else weight.to(dev), label_smoothing=eps,
                                reduction=reduction, pixel_weight=m.to(dev))
        ref.backward(torch.tensor(0.7, device=dev))
        assert torch.equal(loss, ref.detach().cpu()) and torch.equal(grad, zd.grad.cpu()), what
        assert (st["kept"] > 0).all() and (st["kept"] <= st["valid"]).all(), what


# ----------------------------------------------------------------------------------------------- 3. parity with float64
SHAPES = ((2, 5, 7), (1, 16, 16), (3, 9, 13))
# seeds 3000 + 10 C + B; where the float64 distances that decide a selection fall below GAP another seed is taken (the
# assertion in _oracle holds for every case: nothing is left out)
OTHER_SEED = {((1, 8, 16, 16), "hard", t, 85, 0.0, scope): 4000 for t in (0.7, None) for scope in ("batch", "image")}
OTHER_SEED.update({((3, 9, 9, 13), "hard", t, 7, 0.0, "image"): 4000 for t in (0.7, None)})


def selection_variants(hw):
    out = [dict(mode="hard", thresh=t, min_kept=k) for t in (0.7, None) for k in (1, 7, hw // 3, hw)]
    return out + [dict(mode="trim", drop_frac=q) for q in (0.1, 0.25, 0.5)]


@functools.lru_cache(maxsize=None)
def _case(shape, seed):
    return make_case(shape, seed)


def _oracle(shape, seed, sel, scope, full, reduction="mean"):
    """The float64 result, after the assertion (on the CPU) that float32 rounding of a loss cannot move a pixel across the
    selection boundary."""
    z, y, w, p = _case(shape, seed)
    weight, eps, pw = (w.numpy(), 0.1, p.numpy()) if full else (None, 0.0, None)
    res = mined_ce(z.numpy(), y.numpy(), -100, sel["mode"], sel.get("thresh"), sel.get("min_kept", 0), sel.get("drop_frac", 0.0), scope,
                   weight, eps, pw, reduction, upstream=0.7)
    g_rank, g_cap = boundary_gaps(res, sel["mode"], sel.get("thresh"), sel.get("min_kept", 0), sel.get("drop_frac", 0.0), scope)
    assert g_rank >= GAP and g_cap >= GAP, (shape, seed, sel, scope, g_rank, g_cap)
    return res


def parity_seed(shape, sel, scope):
    key = (shape, sel["mode"], sel.get("thresh"), sel.get("min_kept", 0), sel.get("drop_frac", 0.0), scope)
    return OTHER_SEED.get(key, 3000 + 10 * shape[1] + shape[0])


@gpu
@pytest.mark.parametrize("C", (2, 3, 8, 9, 21))
@pytest.mark.parametrize("BHW", SHAPES)
def test_parity_against_float64(dev, BHW, C):
    shape = (BHW[0], C, BHW[1], BHW[2])
    worst = 0.0
    for sel, scope, full in itertools.product(selection_variants(BHW[1] * BHW[2]), ("batch", "image"), (False, True)):
        seed = parity_seed(shape, sel, scope)
        res = _oracle(shape, seed, sel, scope, full)
        z, y, w, p = _case(shape, seed)
        weight, eps, pw = (w, 0.1, p) if full else (None, 0.0, None)
        loss, grad, st = run_mined(dev, z, y, weight, eps, pw, "mean", scope=scope, **sel)
        what = (shape, sel, scope, full)
        assert np.array_equal(st["kept"].numpy(), res["kept"]) and np.array_equal(st["valid"].numpy(), res["n_valid"]), what
        el, eg = rel_err(loss, res["loss"]), rel_err(grad, res["grad"])
        # the threshold is one entry of the loss map: its error is measured like the map's, against the map's largest entry
        # (the k-th largest loss of a well-classified pixel is ~1e-5, where the difference lse - logit has no relative accuracy)
        fin = np.isfinite(res["threshold"])
        assert np.array_equal(np.isfinite(st["threshold"].numpy()), fin), what
        et = float(np.abs(st["threshold"].numpy().astype(np.float64) - res["threshold"])[fin].max(initial=0.0) / np.abs(res["nll"]).max())
        worst = max(worst, el, eg)
        assert el <= REL and eg <= REL and et <= REL, (what, el, eg, et)
    print(f"mined CE parity {shape}: worst rel err {worst:.3e} (bound {REL:.0e})")


# -------------------------------------------------------------------------------------------------------------- 4. ties
@gpu
def test_ties_at_the_threshold_are_all_kept(dev):
    """Every distinct pixel 16 times: the pixels of one group share their loss bit for bit, so rank k falls inside a group."""
    z0, y0, w, _ = make_case((2, 3, 4, 4), 77)
    y0[y0 == -100] = 1
    z, y = z0.repeat(1, 1, 4, 4), y0.repeat(1, 4, 4)
    r0 = mined_ce(z0.numpy(), y0.numpy(), mode="trim")
    d = np.sort(np.unique(r0["nll"]))
    assert d.size == 32 and ((d[1:] - d[:-1]) / d[1:]).min() >= GAP           # the groups themselves are well apart
    for sel, scope, k in ((dict(mode="hard", min_kept=20), "batch", 40), (dict(mode="hard", min_kept=20), "image", 20),
                          (dict(mode="hard", thresh=0.7, min_kept=3), "image", 3), (dict(mode="trim", drop_frac=0.1), "batch", None),
                          (dict(mode="trim", drop_frac=0.3), "image", None)):
        res = mined_ce(z.numpy(), y.numpy(), scope=scope, **sel)
        loss, grad, st = run_mined(dev, z, y, scope=scope, **sel)
        assert np.array_equal(st["kept"].numpy(), res["kept"]), (sel, scope, st["kept"], res["kept"])
        assert (st["kept"] % 16 == 0).all()
        if k is not None:
            assert (st["kept"] > k).all(), (sel, scope, st["kept"])              # inclusive: more than k
        else:
            n = st["valid"].numpy()
            assert (n - st["kept"].numpy() < np.floor(sel["drop_frac"] * n)).all()   # fewer dropped than the fraction allows
        assert rel_err(loss, res["loss"]) <= REL and rel_err(grad, res["grad"] * 0.7) <= REL, (sel, scope)


# ------------------------------------------------------------------------------------------------------------- 5. edges
@gpu
def test_edges(dev):
    from weaklysuperviseddl_amd import ops
    shape = (2, 3, 5, 7)
    z, y, w, p = make_case(shape, 11)
    # every pixel ignored
    yi = torch.full_like(y, -100)
    for sel, scope, kw in itertools.product((dict(mode="hard", thresh=0.7, min_kept=4), dict(mode="hard", min_kept=4),
                                             dict(mode="trim", drop_frac=0.25)), ("batch", "image"),
                                            ({}, {"weight": w, "eps": 0.1, "pw": p})):
        loss, grad, st = run_mined(dev, z, yi, reduction="mean", scope=scope, **sel, **kw)
        assert torch.isnan(loss) and not grad.any() and not torch.isnan(grad).any(), (sel, scope)
        assert not st["kept"].any() and not st["valid"].any() and torch.isposinf(st["threshold"]).all() and not st["selection"].any()
        loss, grad, st = run_mined(dev, z, yi, reduction="sum", scope=scope, **sel, **kw)
        assert loss.item() == 0.0 and not grad.any() and not st["kept"].any(), (sel, scope)
    # every pixel weight 0 is the same thing
    loss, grad, st = run_mined(dev, z, y, pw=torch.zeros_like(p), mode="trim", drop_frac=0.1)
    assert torch.isnan(loss) and not grad.any() and not st["kept"].any()
    # one label that is no class: the pixel keeps its weight and poisons the loss
    yb = y.clone()
    yb[1, 2, 3] = 3
    for sel, reduction in itertools.product((dict(mode="hard", thresh=0.7, min_kept=4), dict(mode="trim", drop_frac=0.25)), ("mean", "sum")):
        loss, _, st = run_mined(dev, z, yb, reduction=reduction, **sel)
        assert torch.isnan(loss), (sel, reduction)
        assert st["selection"][1, 2, 3] == 1.0 and st["valid"].item() == (yb != -100).sum() - 1   # selected, but no candidate of the select
    # selections that keep everything: the LOSS is the plain call's bit for bit; the gradient is, bit for bit, that of the
    # composition - the existing kernel with a pixel weight of ones.  That instantiation of the existing kernel (not touched
    # here) rounds 2 of these 210 gradient entries one ulp away from the instantiation without options (measured on an MI355X:
    # largest difference 9.3e-10 absolute, 1.1e-7 relative), so against the plain call's gradient the bound is REL.
    def reference(**kw):
        zd = z.to(dev).requires_grad_(True)
        ref = ops.cross_entropy(zd, y.to(dev), **kw)
        ref.backward(torch.tensor(0.7, device=dev))
        return ref.detach().cpu(), zd.grad.cpu()

    plain, ones = reference(), reference(pixel_weight=torch.ones(2, 5, 7, device=dev))
    for sel in (dict(mode="trim", drop_frac=0.0), dict(mode="hard", min_kept=35), dict(mode="hard", min_kept=10 ** 9, scope="image")):
        loss, grad, st = run_mined(dev, z, y, **sel)
        assert torch.equal(loss, plain[0]) and torch.equal(loss, ones[0]) and torch.equal(grad, ones[1]), sel
        d = (grad - plain[1]).abs()
        print(f"keep-all {sel}: {int((d != 0).sum())} of {d.numel()} gradient entries differ from the plain call, max {d.max().item():.2e}")
        assert rel_err(grad, plain[1]) <= REL, sel
        assert torch.equal(st["kept"], st["valid"])
    # thresh = 1 caps the threshold at 0: every valid pixel
    _, _, st = run_mined(dev, z, y, mode="hard", thresh=1.0)
    assert torch.equal(st["kept"], st["valid"])
    # min_kept = 0 without thresh: nothing
    loss, grad, st = run_mined(dev, z, y, mode="hard")
    assert torch.isnan(loss) and not grad.any() and not st["kept"].any() and torch.isposinf(st["threshold"]).all()


# 525 312 pixels: the grid-stride case of the weighted tests - every workgroup of the select, of the selection map and of the
# cross entropy loops.  Among half a million losses neighbouring ranks are ~1e-6 apart in the bulk, where float32 rounding
# does move pixels across the boundary (that is no arithmetic error; the selection itself is checked exactly in tests 1 and
# 2): the two runs select in the sparse upper tail, where the assertion of _oracle holds.
BIG = (2, 3, 513, 512)
BIG_RUNS = ((dict(mode="hard", thresh=None, min_kept=12), "batch"), (dict(mode="trim", drop_frac=4.2e-5), "batch"))


@gpu
@pytest.mark.parametrize("run", (0, 1))
def test_grid_stride_size_against_float64(dev, run):
    sel, scope = BIG_RUNS[run]
    res = _oracle(BIG, 5, sel, scope, True)
    z, y, w, p = _case(BIG, 5)
    loss, grad, st = run_mined(dev, z, y, w, 0.1, p, "mean", scope=scope, **sel)
    assert np.array_equal(st["kept"].numpy(), res["kept"]) and np.array_equal(st["valid"].numpy(), res["n_valid"])
    el, eg = rel_err(loss, res["loss"]), rel_err(grad, res["grad"])
    print(f"mined CE {BIG} {sel}: loss {el:.3e}, gradient {eg:.3e} (bound {REL:.0e}), kept {st['kept'].tolist()}")
    assert el <= REL and eg <= REL, (el, eg)


# ------------------------------------------------------------------------------------------------------ 6. planned step
def _planned_and_eager(dev, make_criterion):
    """The pattern of tests/test_hip_weighted_ce.py; also returns the criterion's statistics after every step of both runs."""
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    gen = torch.Generator().manual_seed(2)
    batches = [((torch.rand(4, 3, 64, 64, generator=gen)).to(dev), (torch.rand(4, 64, 64, generator=gen) > 0.5).long().to(dev))
               for _ in range(2)]

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = initialize_model(2, device=dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = make_criterion()
            torch.manual_seed(1234)
            losses, stats = [], []
            for i in range(4):
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
                stats.append((crit.threshold.cpu().clone(), crit.kept.cpu().clone(), crit.valid.cpu().clone()))
            torch.cuda.synchronize()
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st, stats
        finally:
            plan.PLAN_STEP[0] = old

    l0, s0, _, k0 = run(False)
    l1, s1, st, k1 = run(True)
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.replays >= 1, (st.records, st.replays)
    assert l0 == l1 and all(np.isfinite(l0)), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    return k0, k1


@gpu
@pytest.mark.parametrize("which", ("hard", "trim"))
def test_planned_step_is_bit_identical_to_eager(dev, which):
    """The rank comes from a count the replay makes itself: the statistics of the replayed step (the fourth) are the eager
    run's, and they are not those of the step before it - a replay that froze k or the threshold could not equal the eager run.
    (The third step records the plan and verifies it on a probe batch, whose statistics it leaves in the buffers.)"""
    import weaklysuperviseddl_amd.nn as wnn
    if which == "hard":
        k0, k1 = _planned_and_eager(dev, lambda: wnn.MinedCrossEntropyLoss(mode="hard", thresh=0.7, min_kept=256))
    else:
        k0, k1 = _planned_and_eager(dev, lambda: wnn.MinedCrossEntropyLoss(mode="trim", drop_frac=0.25, scope="image"))
    print(f"planned mined step ({which}): kept per step {[k[1].tolist() for k in k0]}, threshold {[k[0].tolist() for k in k0]}")
    for i in (0, 1, 3):                                 # eager, eager, (record + probe), replay
        assert all(torch.equal(a, b) for a, b in zip(k0[i], k1[i])), i
    assert not (torch.equal(k0[3][0], k0[2][0]) and torch.equal(k0[3][1], k0[2][1]))
    assert all((k[1] > 0).all() and (k[1] <= k[2]).all() for k in k0)
    if which == "trim":     # at most floor(0.25 n) of every image's n pixels are dropped
        assert all((k[1] >= k[2] - (k[2].double() * 0.25).floor().long()).all() and (k[2] == 64 * 64).all() for k in k0)


# ---------------------------------------------------------------------------------------------------- 7. default untouched
class _Recorder:
    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._real, name)


@gpu
def test_default_path_does_not_touch_the_new_entry_points(dev, monkeypatch):
    from weaklysuperviseddl_amd import ops, plan
    from weaklysuperviseddl_amd._lib import lib
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer

    def refuse(*a, **k):
        raise AssertionError("the default path called a pixel-mining entry point")

    names = []
    monkeypatch.setattr(ops, "cross_entropy_mined", refuse)
    monkeypatch.setattr(ops, "kth_value", refuse)
    monkeypatch.setattr(ops, "lib", lambda: _Recorder(lib(), names))
    monkeypatch.setattr(plan, "PLAN_STEP", [False])
    torch.manual_seed(0)
    model = initialize_model(2, device=dev).train()
    opt = make_optimizer(model, lr=1e-4)
    x = torch.rand(2, 3, 64, 64, device=dev)
    m = (torch.rand(2, 64, 64, device=dev) > 0.5).long()
    for criterion in (None, torch.nn.CrossEntropyLoss()):
        loss = train_step(model, opt, x, m, criterion=criterion)
        assert torch.isfinite(loss)
    assert "wsdl_softmax_ce_fwd_bwd" in names
    assert not [n for n in names if "kth" in n or "mining" in n], sorted(set(names))
