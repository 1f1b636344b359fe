"""CPU checks of the EMA teacher (no GPU): the float64 oracles of csrc/ema.hip (tests/ema_oracle.py) against the closed form of the
average, the warm-up table, an emulated fused multiply-add and torch's float64 softmax; every host-side refusal of ``FlatEMA`` and
``ops.teacher_targets``; what an optimiser without an EMA reports; the ABI table."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_oracle as O  # noqa: E402


# ---- the update ---------------------------------------------------------------------------------------------------------------
def test_warmup_table():
    """d_k = min(decay, (1 + k) / (10 + k)) for k = 0..20: 0.1, 2/11, ... and the cap at the decay - each side as the float32 the
    device holds, so within 2^-24 relative of the table."""
    want = [(1 + k) / (10 + k) for k in range(21)]
    assert want[0] == 0.1 and want[1] == 2 / 11 and abs(want[20] - 0.7) < 1e-15
    for decay in (0.5, 0.999):
        d32 = float(np.float32(decay))
        got = [O.decay_at(decay, True, k) for k in range(21)]
        assert got == [min(d32, float(np.float32(w))) for w in want]
        assert all(abs(g - min(decay, w)) <= 2.0 ** -24 * w for g, w in zip(got, want))
        assert [O.decay_at(decay, False, k) for k in range(21)] == [d32] * 21
    assert O.decay_at(0.5, True, 8) == 0.5 and O.decay_at(0.5, True, 7) == float(np.float32(8 / 17))      # (1 + 8) / 18 = 0.5: the cap takes over
    from weaklysuperviseddl_amd import ema
    assert [ema.warmup_decay(0.999, k) for k in range(21)] == [O.decay_at(0.999, True, k) for k in range(21)]


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_oracle_against_the_closed_form(decay):
    """e_n = d^n e_0 + (1 - d) sum_k d^(n-1-k) p_k for a constant d; the float32 variant stays within n roundings of it."""
    rng = np.random.default_rng(0)
    n, steps = 257, 30
    e0 = rng.standard_normal(n).astype(np.float32)
    ps = [rng.standard_normal(n).astype(np.float32) + 0.05 * k for k in range(steps)]
    d = float(np.float32(decay))
    e64, e32 = e0.astype(np.float64), e0.copy()
    for k, p in enumerate(ps):
        e64 = O.ema_update(e64, p, decay, False, k)
        e32 = O.ema_update32(e32, p, decay, False, k)
    closed = d ** steps * e0.astype(np.float64) + (1 - d) * sum(d ** (steps - 1 - k) * p.astype(np.float64) for k, p in enumerate(ps))
    scale = np.abs(closed).max()
    assert np.abs(e64 - closed).max() <= 1e-13 * scale
    assert np.abs(e32 - closed).max() <= steps * 2.0 ** -24 * scale * 2
    # with warm-up the first update is mostly the parameters: d_0 = 0.1, as a float32
    first = O.ema_update(e0, ps[0], decay, True, 0)
    d0 = float(np.float32(0.1))
    # (two evaluation orders: a few roundings at the size of the operands, not of a result that may cancel)
    size = np.maximum(np.abs(e0), np.abs(ps[0])).astype(np.float64)
    assert (np.abs(first - (d0 * e0.astype(np.float64) + (1.0 - d0) * ps[0].astype(np.float64))) <= 4 * 2.0 ** -52 * size).all()


def test_decay_zero_is_a_copy():
    e, p = O.flat_data(1027, "huge_e", 1)
    assert np.array_equal(O.ema_update32(e, p, 0.0, False, 0), p)
    assert np.array_equal(O.ema_update_fma(e, p, 0.0, False, 0).astype(np.float32), p)
    # through the formula it would not be: e + (p - e) loses p below e's last place
    assert not np.array_equal((e.astype(np.float64) + (p.astype(np.float64) - e.astype(np.float64))).astype(np.float32), p)


@pytest.mark.parametrize("kind", O.DATA_KINDS)
def test_fused_and_unfused_oracle_agree_within_the_cap(kind):
    """The device evaluates fma(a, p - e, e); numpy's multiply-add is unfused.  After the rounding to float32 the two differ at no
    more than 10 elements per million, never by more than one ulp, on the inputs the GPU test uses (measured: 0 of 20971520 for
    each kind of data).

    This holds because the decay of an update is a float32 also during the warm-up.  With the ratio (1 + k) / (10 + k) kept in
    double, a = 9 / (10 + k) is a 53-bit rational with a small denominator, float32 inputs are dyadic, and the exact a (p - e) + e
    lands ON a float32 tie for a few elements per thousand (k = 0: every p - e whose significand is a multiple of 20); the one
    rounding of the product then decides which way the tie breaks, and at scale 1 the two evaluations differed at 13656 of
    20971520 results (651 per million: 3047 of 2^20 at k = 0, 1301 at k = 1, 303 at k = 9, 3 at k = 1000).  The second half of the
    test keeps that finding: the double ratio still breaks the cap."""
    n = 1 << 20
    e, p = O.flat_data(n, kind, 7)
    bad = total = 0
    for decay, warmup, k in O.flat_settings(4):
        a = O.ema_update(e, p, decay, warmup, k).astype(np.float32)
        b = O.ema_update_fma(e, p, decay, warmup, k).astype(np.float32)
        d = O.ulp_distance(a, b)
        assert d.max() <= 1
        bad += int((d != 0).sum())
        total += n
    assert bad <= 10e-6 * total, (bad, total)
    if kind == "unit":
        a_double = 1.0 - 1.0 / 10.0                     # k = 0 with the warm-up ratio in double
        d = p.astype(np.float64) - e.astype(np.float64)
        flips = O.ulp_distance((e + a_double * d).astype(np.float32), O.fma_emulated(a_double, d, e.astype(np.float64)).astype(np.float32))
        assert (flips != 0).sum() > 1000e-6 * n


def test_two_prod_is_exact():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(200), rng.standard_normal(200) * 1e5
    x, y = O._two_prod(a, b)
    for i in range(200):
        assert Fraction(float(a[i])) * Fraction(float(b[i])) == Fraction(float(x[i])) + Fraction(float(y[i]))


# ---- label correction ---------------------------------------------------------------------------------------------------------
def _t(logits, labels, tau, mode="replace"):
    return O.teacher_targets(np.asarray(logits, np.float32), np.asarray(labels, np.int64), tau, mode)


def test_teacher_oracle_against_torch_softmax():
    logits, labels = O.teacher_case((2, 21, 9, 11), "mixed", 5)
    out, conf, counts, p64 = O.teacher_targets(logits, labels, 0.6)
    lg = torch.from_numpy(logits).double()
    finite = torch.isfinite(lg).all(dim=1)
    p, t = torch.softmax(lg, dim=1).max(dim=1)
    ok = finite.numpy()
    assert np.abs(p64[ok] - p.numpy()[ok]).max() < 1e-14 and not p64[~ok].any()
    keep = labels != -100
    assert np.array_equal(conf[keep & ok], p.numpy()[keep & ok].astype(np.float32)) and not conf[~keep].any() and not conf[~ok].any()
    flip = ok & keep & (conf >= np.float32(0.6)) & (t.numpy() != labels)
    assert np.array_equal(out, np.where(flip, t.numpy(), labels))
    assert counts.tolist() == [int((keep & ~flip).sum()), int(flip.sum()), int((~keep).sum())] and counts.sum() == labels.size


def test_teacher_oracle_hand_made_cases():
    # a tie takes the first class: p = 0.5 exactly
    out, conf, counts, _ = _t([[[[1.0]], [[1.0]]]], [[[1]]], 0.5)
    assert out.item() == 0 and conf.item() == 0.5 and counts.tolist() == [0, 1, 0]
    # tau = 0: every finite pixel that disagrees is corrected; tau > 1: the input comes back
    lg = np.asarray([[[[0.1, 0.0]], [[0.0, 0.1]]]], np.float32)
    assert _t(lg, [[[1, 0]]], 0.0)[0].tolist() == [[[0, 1]]]
    out, conf, counts, _ = _t(lg, [[[1, 0]]], 1.5)
    assert out.tolist() == [[[1, 0]]] and counts.tolist() == [2, 0, 0] and (conf > 0.5).all()
    # non-finite logits: never confident, conf 0, whatever tau
    for bad in (np.nan, np.inf, -np.inf):
        out, conf, counts, _ = _t([[[[bad]], [[3.0]]]], [[[0]]], 0.0)
        assert out.item() == 0 and conf.item() == 0.0 and counts.tolist() == [1, 0, 0]
    # gaps of +-40: p = 1 to float32 on one side, exp(-40) does not disturb it on the other
    out, conf, _, p64 = _t([[[[40.0, -40.0]], [[0.0, 0.0]]]], [[[1, 0]]], 0.9)
    assert out.tolist() == [[[0, 1]]] and conf.tolist() == [[[1.0, 1.0]]] and (p64 <= 1.0).all()
    # all pixels ignored; "ignore" mode writes the ignore value
    out, conf, counts, _ = _t(lg, [[[-100, -100]]], 0.0)
    assert out.tolist() == [[[-100, -100]]] and not conf.any() and counts.tolist() == [0, 0, 2]
    assert _t(lg, [[[1, 1]]], 0.0, "ignore")[0].tolist() == [[[-100, 1]]]


@pytest.mark.parametrize("shape", O.TEACHER_SHAPES)
def test_teacher_inputs_stay_inside_the_exemption_cap(shape):
    """The GPU test may exempt pixels whose float64 p lies within 2^-22 of tau, at most 0.1 % of a case: a float32 evaluation of the
    contract agrees with the float64 oracle everywhere else, and the inputs have at most that share of such pixels."""
    for content in O.TEACHER_CONTENTS:
        logits, labels = O.teacher_case(shape, content, 11)
        for tau in O.TEACHER_TAUS:
            for mode in ("replace", "ignore"):
                out, _conf, counts, p64 = O.teacher_targets(logits, labels, tau, mode)
                out32, counts32 = O.teacher_targets32(logits, labels, tau, mode)
                near = (p64 > 0) & (np.abs(p64 - float(np.float32(tau))) <= O.TAU_BAND)     # (p = 0: a non-finite pixel, never confident)
                assert near.sum() <= 1e-3 * near.size, (shape, content, tau, int(near.sum()))
                assert np.array_equal(out[~near], out32[~near])
                assert np.abs(counts - counts32).max() <= near.sum()
                if content == "agree":
                    assert np.array_equal(out, labels) and counts[1] == 0


# ---- host logic ---------------------------------------------------------------------------------------------------------------
def _net(width=4):
    from weaklysuperviseddl_amd import nn as wnn
    return torch.nn.Sequential(wnn.Conv2d(3, width, 3, padding=1, bias=False), wnn.BatchNorm2d(width))


def test_flat_ema_refusals_come_before_any_device_call():
    from weaklysuperviseddl_amd import ema, ops, optim
    student = _net()
    opt = optim.FlatAdam(student.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="same parameters"):
        ema.FlatEMA(opt, student, torch.nn.Sequential(_net()[0]))
    with pytest.raises(ValueError, match="student .* teacher"):
        ema.FlatEMA(opt, student, _net(width=8))
    with pytest.raises(ValueError, match="second instance"):
        ema.FlatEMA(opt, student, student)
    other = _net()
    other[1].running_mean = other[1].running_mean.double()
    with pytest.raises(ValueError, match="buffer 1.running_mean"):
        ema.FlatEMA(opt, student, other)
    for decay in (-0.1, 1.0, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="decay"):
            ema.FlatEMA(opt, student, _net(), decay=decay)
    with pytest.raises(ValueError, match="'ema' or 'copy'"):
        ema.FlatEMA(opt, student, _net(), buffers="swa")
    with pytest.raises(ValueError, match="owns none"):
        ema.FlatEMA(optim.FlatAdam(_net().parameters(), lr=0.1), student, _net())
    # everything right but the place: refused too, and nothing was attached meanwhile
    with pytest.raises(ops.WsdlError, match="no CPU fallback"):
        ema.FlatEMA(opt, student, _net())
    assert opt.ema is None


def test_optimiser_without_an_ema_reports_what_it_always_did():
    from weaklysuperviseddl_amd import ops, optim

    def ps():
        return [torch.nn.Parameter(torch.randn(4))]
    opt = optim.FlatAdam(ps(), lr=0.1)
    assert opt.ema is None and opt.launch_key() == (None, False, False)
    assert [id(t) for t in opt.state_tensors()] == [id(opt.flat_param), id(opt.exp_avg), id(opt.exp_avg_sq)]
    assert optim.FlatSGD(ps(), lr=0.1, momentum=0.9).launch_key() == (ops.FLAT_SGD, False, False)
    assert optim.FlatAdamW(ps(), lr=0.1, skip_nonfinite=True).launch_key() == (ops.FLAT_ADAMW, True, False)

    class Stub:                                            # what FlatEMA adds, without a device
        def launch_key(self):
            return ("ema", 1, "ema", 2)

        def state_tensors(self):
            return ["e", "b", "s"]

        def sync_hyper(self):
            pass
    opt.ema = Stub()
    assert opt.launch_key() == (None, False, False, ("ema", 1, "ema", 2)) and opt.state_tensors()[-3:] == ["e", "b", "s"]
    # GraphedTrainStep compares launch_key() with the default triple: an attached EMA is refused there
    src = inspect.getsource(__import__("weaklysuperviseddl_amd.graph", fromlist=["x"]))
    assert "launch_key() != (None, False, False)" in src


def test_teacher_targets_refusals_on_host():
    from weaklysuperviseddl_amd import ops
    lg, lab = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    bad = [
        (dict(mode="soften"), "'replace' or 'ignore'"),
        (dict(tau="0.9"), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=True), "tau"), (dict(tau=torch.zeros(2)), "tau"),
        (dict(tau=torch.zeros(1, dtype=torch.float64)), "tau"),
        (dict(ignore_index=1.5), "ignore_index"),
        (dict(logits=lg[0]), "rank 4"), (dict(logits=lg.double()), "float32"), (dict(labels=lab.int()), "int64"),
        (dict(labels=lab[:, :3]), "must be"), (dict(logits=torch.zeros(1, 65, 2, 2), labels=torch.zeros(1, 2, 2, dtype=torch.int64)), "at most 64"),
        (dict(logits=torch.zeros(0, 3, 4, 5), labels=torch.zeros(0, 4, 5, dtype=torch.int64)), "empty"),
        (dict(out=torch.zeros(2, 4, 5)), "out must be"), (dict(out=lab), "out shares memory with labels"),
        (dict(conf=torch.zeros(2, 4, 4)), "conf must be"), (dict(counts=torch.zeros(3)), "counts must be"),
        (dict(conf=lg[:, 0]), "conf must be"), (dict(conf="yes"), "conf must be True, False"),
    ]
    for kw, msg in bad:
        args = dict(logits=lg, labels=lab)
        args.update(kw)
        with pytest.raises(ops.WsdlError, match=msg):
            ops.teacher_targets(**args)
    shared = torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(ops.WsdlError, match="shares memory"):
        ops.teacher_targets(lg, lab, out=shared, counts=shared.view(-1)[:3])
    with pytest.raises(ops.WsdlError, match="no CPU fallback"):         # the place last
        ops.teacher_targets(lg, lab)
    with pytest.raises(ops.WsdlError, match="device tensor"):
        ops.flat_ema(torch.zeros(4), torch.zeros(4), torch.zeros(2), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ops.WsdlError, match="'ema' or 'copy'"):
        ops.ema_table(torch.zeros(24, dtype=torch.uint8), 1, None, None, None, mode="swa")


def test_new_symbols_are_in_the_header_and_bound():
    from weaklysuperviseddl_amd import _build, _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "wsdl_hip.h")).read()
    for name, nargs in (("wsdl_flat_ema", 8), ("wsdl_ema_table", 8), ("wsdl_teacher_targets", 13)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib(), name)
    assert re.search(r"#define WSDL_TEACHER_MAX_CLASSES %d\b" % ops.TEACHER_MAX_CLASSES, src)
    assert ops.EMA_ENTRY_DTYPE.itemsize == 24 and "wsdl_ema_entry" in src
    assert "ema.hip" in _build.SOURCES


def test_callers_take_the_ema_additively():
    import importlib
    S = importlib.import_module("weaklysuperviseddl_amd.TraditionalModel.SegmentationModel")
    A = importlib.import_module("weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss")
    sig = inspect.signature(S.train_segmentation_model).parameters
    assert sig["ema"].kind is inspect.Parameter.KEYWORD_ONLY and sig["ema"].default is None
    sig = inspect.signature(A.run_alternating_training).parameters
    assert list(sig)[-1] == "ema" and sig["ema"].default is None
    sig = inspect.signature(A.refine_dataset).parameters
    assert sig["teacher_kwargs"].default is None
    sig = inspect.signature(S.train_step_mean_teacher).parameters
    assert list(sig)[:6] == ["model", "ema", "optimizer", "images", "masks", "criterion"]
    assert [sig[k].default for k in ("tau", "mode", "weight_by_conf")] == [0.9, "ignore", False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("tau", "mode", "weight_by_conf"))
    assert "ema" not in inspect.signature(S.train_step).parameters
    with pytest.raises(ValueError, match="'ignore' mode"):
        A.refine_dataset(None, None, method="teacher", teacher_kwargs={"mode": "ignore"})
