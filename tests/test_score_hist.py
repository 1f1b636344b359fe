"""The score-histogram oracle (tests/score_hist_oracle.py) held to independent formulations, the host reductions on hand-made
counts, and every host-side refusal of ``check_score_hist_options`` - no device anywhere in this file."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_hist_oracle as O  # noqa: E402

from weaklysuperviseddl_amd import WsdlError, ops  # noqa: E402

F = np.float32
# the three tables whose arithmetic bin guess the issue counted as off by one: (bins, lo, hi)
NEIGHBOUR_TABLES = [(1000, 0.0, 1.0), (1024, -3.0, 5.0), (7, 0.1, 0.7)]


def edge_neighbours(edges):
    """every edge and its two float32 neighbours"""
    e = np.asarray(edges, dtype=F)
    return np.concatenate([np.nextafter(e, F(-np.inf)), e, np.nextafter(e, F(np.inf))]).astype(F)


def arithmetic_slots(v, lo, hi, nb):
    """the float32 guess floor((v - lo) * nb / (hi - lo)) an uncorrected kernel would bin by (in-range values only)"""
    v = np.asarray(v, dtype=F)
    k = np.floor((v - F(lo)) * (F(nb) / (F(hi) - F(lo)))).astype(np.int64)
    return 1 + np.clip(k, 0, nb - 1)


def _loop_slot(v, edges):
    nb = len(edges) - 1
    if v != v:
        return nb + 2
    if v < edges[0]:
        return 0
    if v >= edges[nb]:
        return nb + 1
    for k in range(nb):
        if edges[k] <= v < edges[k + 1]:
            return 1 + k
    raise AssertionError


def test_uniform_edges_values():
    e = ops.uniform_edges(0.0, 1.0, 256)
    assert e.dtype == F and e.shape == (257,) and e[0] == 0 and e[-1] == 1
    assert np.array_equal(e, (np.arange(257) / 256).astype(F))             # k / 256 is exact
    e = ops.uniform_edges(0.1, 0.7, 7)
    assert np.array_equal(e, np.linspace(0.1, 0.7, 8).astype(F)) and np.array_equal(e, O.uniform_edges(0.1, 0.7, 7))
    assert e[0] == F(0.1) and e[-1] == F(0.7) and (np.diff(e) > 0).all()
    # rounded ONCE from float64: every edge is the float32 nearest to the exact k / bins point
    e = ops.uniform_edges(-3.0, 5.0, 1000)
    exact = [Fraction(-3) + Fraction(8 * k, 1000) for k in range(1001)]
    assert all(abs(Fraction(float(x)) - q) <= abs(Fraction(float(np.nextafter(x, F(np.inf)))) - Fraction(float(x))) / 2 + Fraction(1, 2 ** 50)
               for x, q in zip(e, exact))
    for bad in ((1.0, 1.0, 4), (2.0, 1.0, 4), (0.0, float("inf"), 4), (0.0, 1.0, 0), (0.0, 1.0, 1025), (0.0, 1.0, 2.5)):
        with pytest.raises(WsdlError):
            ops.uniform_edges(*bad)


def test_slots_and_sums_against_a_pixel_loop():
    rng = np.random.default_rng(0)
    edges = np.array([-0.5, 0.0, 0.125, 0.5, 2.0], dtype=F)
    v = np.concatenate([rng.uniform(-1, 3, 300).astype(F), edge_neighbours(edges),
                        np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45], dtype=F)])
    g = rng.integers(-1, 4, v.shape).astype(np.int64)                       # 3 is outside [0, 3): not counted; so is -1
    counts, sums = O.histogram(v[None], g[None], edges, num_groups=3, want_sums=True)
    want_c, want_s = np.zeros((3, 7), dtype=np.int64), np.zeros((3, 7), dtype=np.int64)
    for x, gi in zip(v.tolist(), g.tolist()):
        if 0 <= gi < 3:
            s = _loop_slot(F(x), edges)
            want_c[gi, s] += 1
            if 1 <= s <= 4:
                want_s[gi, s] += int(Fraction(float(F(x))) * 2 ** 24)       # exact product, truncated toward zero
    assert np.array_equal(counts[0], want_c) and np.array_equal(sums[0], want_s)
    assert counts.sum() == ((g >= 0) & (g < 3)).sum()
    assert O.slots(np.array([-0.0], dtype=F), edges)[0] == 2               # -0.0 compares as 0
    assert O.slots(np.array([np.inf, np.nan], dtype=F), edges).tolist() == [5, 6]


def test_histogram_against_np_histogram_and_segments():
    rng = np.random.default_rng(1)
    v = rng.uniform(0, 1, (3, 5, 41)).astype(F)
    v[v == 1] = 0.5                                                         # np.histogram closes its last bin
    edges = O.uniform_edges(0, 1, 16)
    per = O.histogram(v, None, edges, per_image=True)
    for b in range(3):
        assert np.array_equal(per[b, 0, 1:-2], np.histogram(v[b], bins=edges)[0])
        assert per[b, 0, 0] == per[b, 0, -1] == per[b, 0, -2] == 0
    assert np.array_equal(O.histogram(v, None, edges, per_image=False)[0], per.sum(axis=0))


@pytest.mark.parametrize("nb,lo,hi", NEIGHBOUR_TABLES)
def test_arithmetic_guess_is_wrong_on_the_edge_neighbours(nb, lo, hi):
    """The contents tests/test_hip_score_hist.py bins at these tables defeat a kernel that trusts floor((v - lo) * nb / (hi - lo)):
    it differs from the comparison rule on them, so the GPU test cannot pass without the correction."""
    edges = O.uniform_edges(lo, hi, nb)
    v = edge_neighbours(edges)
    s = O.slots(v, edges)
    inside = (s >= 1) & (s <= nb)
    wrong = (arithmetic_slots(v[inside], lo, hi, nb) != s[inside]).sum()
    assert wrong >= 1, (nb, lo, hi)
    # and the comparison rule puts an edge into the bin it opens, its lower neighbour into the one before
    assert np.array_equal(O.slots(edges, edges), np.arange(1, nb + 2))
    assert np.array_equal(O.slots(np.nextafter(edges, F(-np.inf)), edges), np.arange(0, nb + 1))


def test_curves_against_a_threshold_loop():
    rng = np.random.default_rng(2)
    edges = O.uniform_edges(0, 1, 12)
    v = rng.uniform(-0.2, 1.2, (2, 200)).astype(F)
    v[0, :5] = [np.nan, np.inf, -np.inf, 1.0, 0.0]
    v[:, 5:18] = edges[None]
    gt = rng.integers(0, 3, v.shape).astype(np.int64)                      # 2 = not counted
    cv = O.curves(O.histogram(v, gt, edges, num_groups=2))
    for b in range(2):
        keep = gt[b] < 2
        for k, t in enumerate(edges):
            with np.errstate(invalid="ignore"):
                pred = (v[b] >= t)[keep]
            pos = (gt[b] == 1)[keep]
            want = [np.logical_and(pred, pos).sum(), np.logical_and(pred, ~pos).sum(), np.logical_and(~pred, pos).sum(),
                    np.logical_and(~pred, ~pos).sum()]
            assert cv[b, k].tolist() == want, (b, k)
            assert np.logical_or(pred, pos).sum() == cv[b, k, :3].sum()


def _fraction_otsu(bin_index, nb):
    """first maximum over k = 0 .. nb - 2 of the two-class between variance w0 w1 (mu0 - mu1)^2 of the pixels' bin indices, exact"""
    best, kb = None, -1
    n = len(bin_index)
    for k in range(nb - 1):
        a, b = [i for i in bin_index if i <= k], [i for i in bin_index if i > k]
        if not a or not b:
            continue
        q = Fraction(len(a), n) * Fraction(len(b), n) * (Fraction(sum(a), len(a)) - Fraction(sum(b), len(b))) ** 2
        if best is None or q > best:
            best, kb = q, k
    return kb, best


def test_otsu_against_exact_two_class_variance():
    rng = np.random.default_rng(3)
    for trial in range(40):
        nb = int(rng.integers(2, 40))
        edges = O.uniform_edges(0, 1, nb)
        n = int(rng.integers(2, 120))
        idx = rng.integers(0, nb, n) if trial % 3 else rng.choice([1 % nb, nb - 1], n)      # some bimodal with empty bins between
        counts = np.zeros((1, 1, nb + 3), dtype=np.int64)
        np.add.at(counts[0, 0], 1 + idx, 1)
        k, t, q = O.otsu(counts, edges)
        kb, best = _fraction_otsu(idx.tolist(), nb)
        assert k[0] == kb, (trial, k, kb)
        if kb >= 0:
            assert t[0] == edges[kb + 1]
            # q = D^2 / (w0 w1) = n^2 * w0 w1 (mu0 - mu1)^2 with w in fractions of n
            assert q[0] == pytest.approx(float(best * n * n), rel=1e-12)
        else:
            assert t[0] == F(0.5) and q[0] == 0.0


def test_otsu_fallback_plateau_and_group_subset():
    edges = O.uniform_edges(0, 1, 8)
    c = np.zeros((3, 2, 11), dtype=np.int64)
    c[0, 0, 3] = 50                                                         # one occupied bin: the fallback
    c[1, 0, 2], c[1, 1, 7] = 10, 10                                         # bins 1 and 6: q is flat over k = 1 .. 5, the first wins
    c[2, 0, 1], c[2, 0, 2], c[2, 1, 8] = 4, 4, 100                          # group 0 alone: bins 0 and 1
    k, t, q = O.otsu(c, edges, fallback=0.25)
    assert k.tolist() == [-1, 1, 1] and t[0] == F(0.25) and t[1] == edges[2]
    k0, t0, _ = O.otsu(c, edges, groups=[0], fallback=0.25)
    assert k0.tolist() == [-1, -1, 0] and t0[2] == edges[1]
    c[:, :, 0] = c[:, :, -1] = c[:, :, -2] = 999                            # the outer slots and NaN take no part
    assert O.otsu(c, edges, fallback=0.25)[0].tolist() == [-1, 1, 1]


def test_host_reductions_on_hand_made_counts():
    # TP FP FN TN at three thresholds; the last one predicts nothing and there the union of segment 1 is empty
    cv = np.array([[[4, 4, 0, 0], [3, 1, 1, 3], [0, 0, 4, 4]],
                   [[0, 8, 0, 0], [0, 2, 0, 6], [0, 0, 0, 8]]], dtype=np.int64)
    edges = np.array([0.0, 0.5, 1.0], dtype=F)
    iou = ops.iou_curve_from_counts(cv)
    assert np.array_equal(iou, O.iou_curve(cv)) and iou[1, 2] == 1.0 and iou[0, 1] == 3 / 5 and iou[1, 0] == 0.0
    assert ops.iou_curve_from_counts(cv, empty=0.0)[1, 2] == 0.0
    assert ops.iou_curve_from_counts(cv, eps=1e-8)[0, 1] == 3 / (5 + 1e-8) and ops.iou_curve_from_counts(cv, eps=1e-8)[1, 2] == 0.0
    assert np.array_equal(ops.accuracy_curve_from_counts(cv), np.array([[0.5, 0.75, 0.5], [0.0, 0.75, 1.0]]))
    # dataset: pooled TP / union = 4/16, 3/7, 0/4 -> threshold 0.5; mean of images: (0.5+0)/2, (0.6+0)/2, (0+1)/2 -> threshold 1.0
    assert ops.best_threshold(cv, edges, "iou", "dataset") == (0.5, 3 / 7, 1)
    assert ops.best_threshold(cv, edges, "iou", "mean_image") == (1.0, 0.5, 2)
    t, f, k = ops.best_threshold(cv, edges, "f", "dataset")
    assert (t, k) == (0.5, 1) and f == pytest.approx(O.fbeta_curve(cv.sum(axis=0))[1]) and ops.max_fbeta(cv) == (f, 1)
    with pytest.raises(WsdlError):
        ops.best_threshold(cv, edges, "dice")
    with pytest.raises(WsdlError):
        ops.best_threshold(cv, edges[:2])
    p, r = ops.pr_curve(cv)
    assert np.array_equal(p, O.pr(cv)[0]) and np.array_equal(r, O.pr(cv)[1]) and p[2] == 1.0 and r.tolist() == [1.0, 0.75, 0.0]
    # AP: scores 0.05 .. 0.95 in ten bins; a perfect ranking (all positives above all negatives) and its reverse
    e10 = O.uniform_edges(0, 1, 10)
    v = (np.arange(10) / 10 + 0.05).astype(F)[None]
    perfect, reverse = (np.arange(10) >= 6).astype(np.int64)[None], (np.arange(10) < 4).astype(np.int64)[None]
    ap_p = ops.average_precision(O.curves(O.histogram(v, perfect, e10, num_groups=2)))
    ap_r = ops.average_precision(O.curves(O.histogram(v, reverse, e10, num_groups=2)))
    assert ap_p == 1.0 and ap_p == O.average_precision(O.curves(O.histogram(v, perfect, e10, num_groups=2)))
    # reversed: the k-th positive is recalled with 6 negatives above it: mean of (1/7, 2/8, 3/9, 4/10)
    assert ap_r == pytest.approx((1 / 7 + 2 / 8 + 3 / 9 + 4 / 10) / 4, rel=1e-12) and ap_r < 0.31


def test_mae_ece_and_tau_on_hand_made_tables():
    rng = np.random.default_rng(4)
    e = O.uniform_edges(0, 1, 10)
    v = rng.uniform(0, 1, (2, 300)).astype(F)
    v[0, :4] = [1.0, 0.0, 1.0, np.nan]
    gt = rng.integers(0, 2, v.shape).astype(np.int64)
    counts, sums = O.histogram(v, gt, e, num_groups=2, want_sums=True)
    assert ops.mae_from_sums(counts, sums) == pytest.approx(O.mae(v, gt), rel=1e-12)
    assert ops.mae_from_sums(np.zeros((1, 2, 13)), np.zeros((1, 2, 13))) == 0.0
    # a calibrated table: in the bin of confidence (k + 0.5) / 10 exactly that share of 20 pixels is right -> ECE 0
    conf = np.repeat((np.arange(5, 10) / 10 + 0.05).astype(F), 20)
    conf = (np.round(conf.astype(np.float64) * 2 ** 24) / 2 ** 24).astype(F)
    right = np.concatenate([(np.arange(20) < round(20 * (k / 10 + 0.05))).astype(np.int64) for k in range(5, 10)])
    counts, sums = O.histogram(conf[None], right[None], e, num_groups=2, want_sums=True)
    ece, acc, cf, cnt = ops.ece_from_counts(counts, sums)
    assert ece == pytest.approx(0.0, abs=1e-7) and cnt.tolist() == [0] * 5 + [20] * 5 and np.isnan(acc[:5]).all() and np.isnan(cf[:5]).all()
    assert np.allclose(acc[5:], [0.55, 0.65, 0.75, 0.85, 0.95]) and np.allclose(cf[5:], acc[5:], atol=1e-7)
    o_ece, o_acc, o_cf, o_cnt = O.ece(conf, right, 10)
    assert ece == pytest.approx(o_ece, abs=1e-12) and np.array_equal(cnt, o_cnt) and np.allclose(acc[5:], o_acc[5:]) and np.allclose(cf[5:], o_cf[5:])
    # an over-confident table, with confidences of exactly 1 (the slot above the last edge joins the last bin)
    conf2 = np.concatenate([conf, np.ones(10, dtype=F)])
    right2 = np.concatenate([right, np.zeros(10, dtype=np.int64)])
    counts2, sums2 = O.histogram(conf2[None], right2[None], e, num_groups=2, want_sums=True)
    ece2, _acc2, _cf2, cnt2 = ops.ece_from_counts(counts2, sums2)
    assert cnt2[-1] == 30 and ece2 == pytest.approx(O.ece(conf2, right2, 10)[0], abs=1e-12) and ece2 > 0.05
    # tau: accuracy at and above 0.5 .. 0.9 is 0.75, 0.8, 0.85, 0.9, 0.95
    assert ops.tau_for_precision(counts, e, 0.9) == float(e[8]) == O.tau_for_precision(conf, right, e, 0.9)
    assert ops.tau_for_precision(counts, e, 0.7) == float(e[0]) == O.tau_for_precision(conf, right, e, 0.7)
    assert ops.tau_for_precision(counts, e, 0.96) is None and O.tau_for_precision(conf, right, e, 0.96) is None


def test_confidence_planes_float32_oracle_within_its_bound():
    """The yardstick of the device test, on the CPU: the float32 evaluation of the softmax maximum stays within
    max(4 x its own distance to float64, 2^-23 |value|) trivially; what has to hold is that at most 0.1 % of the pixels have a
    top-two margin so small that the arg-max is exempt - with the contents the device test uses."""
    for C_, seed in ((2, 0), (3, 1), (21, 2), (64, 3)):
        z = confidence_logits(C_, seed)
        c64, p64 = O.confidence_planes(z, np.float64)
        c32, p32 = O.confidence_planes(z, np.float32)
        fin = np.isfinite(c64)
        bound = np.maximum(4 * np.abs(c32.astype(np.float64) - c64), 2.0 ** -23 * np.abs(c64))
        exempt = confidence_exempt(z, bound)
        assert exempt[fin].mean() <= 1e-3, (C_, exempt[fin].mean())
        assert np.array_equal(p32[fin & ~exempt], p64[fin & ~exempt])
        assert np.isnan(c64[~fin]).all() and (~fin).sum() >= 1


def confidence_logits(C_, seed, B=2, H=24, W=36):
    """logits on a 1/8 grid (ties are exact or at least 1/8 apart), with gaps of +-40, one non-finite logit per kind"""
    rng = np.random.default_rng(100 + seed)
    z = (rng.integers(-24, 25, (B, C_, H, W)) / 8.0).astype(F)
    z[0, 0, :2] += 40.0
    z[0, C_ - 1, 2:4] -= 40.0
    z[1, 0, 0, 0], z[1, C_ - 1, 0, 1], z[1, 0, 0, 2] = np.nan, np.inf, -np.inf
    return z


def confidence_exempt(z, bound):
    """pixels whose top-two softmax margin does not exceed twice the bound: their arg-max is not compared"""
    zz = np.where(np.isfinite(z), z, -1e30).astype(np.float64)
    p = np.exp(zz - zz.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    top = np.sort(p, axis=1)[:, -2:]
    first = np.argmax(zz, axis=1)
    tie_is_first = np.ones(first.shape, dtype=bool)                        # an exact tie keeps the FIRST arg-max: not exempt
    return ((top[:, 1] - top[:, 0]) <= 2 * bound) & ~((top[:, 1] == top[:, 0]) & tie_is_first)


# ---- refusals, all without a device --------------------------------------------------------------------------------------------
def _refused(**kw):
    with pytest.raises(WsdlError) as e:
        ops.check_score_hist_options(**kw)
    return str(e.value)


def test_every_refusal_is_reached_without_a_device():
    s = torch.zeros(2, 4, 5)
    g = torch.zeros(2, 4, 5, dtype=torch.int64)
    e = torch.tensor([0.0, 0.5, 1.0])
    assert "rank" in _refused(scores=torch.zeros(5))
    assert "float32" in _refused(scores=s.double())
    assert "empty" in _refused(scores=torch.zeros(2, 0))
    assert "tensor" in _refused(scores=[[1.0]])
    assert "int64" in _refused(scores=s, groups=g.int())
    assert "must be" in _refused(scores=s, groups=g[:, :3])
    assert "bools" in _refused(scores=s, per_image=1)
    assert "bins" in _refused(scores=s, bins=0)
    assert "bins" in _refused(scores=s, bins=1025)
    assert "bins" in _refused(scores=s, bins=16.0)
    assert "range" in _refused(scores=s, range=(1.0, 1.0))
    assert "range" in _refused(scores=s, range=(0.0, float("nan")))
    assert "distinct" in _refused(scores=s, range=(1.0, 1.0 + 2.0 ** -20), bins=1024)
    assert "num_groups" in _refused(scores=s, num_groups=0)
    assert "num_groups" in _refused(scores=s, num_groups=33)
    assert "slots" in _refused(scores=s, num_groups=4, bins=1024)          # 4 x 1027 > 4096
    assert "slots" in _refused(scores=s, num_groups=32, bins=126)          # 32 x 129 = 4128
    assert "rank" in _refused(scores=s, edges=e[None])
    assert "float32" in _refused(scores=s, edges=e.double())
    assert "edges" in _refused(scores=s, edges=torch.zeros(1))
    assert "edges" in _refused(scores=s, edges=torch.arange(1026.0))
    assert "ascending" in _refused(scores=s, edges=torch.tensor([0.0, 0.5, 0.5]))
    assert "ascending" in _refused(scores=s, edges=torch.tensor([0.0, 1.0, 0.5]))
    assert "finite" in _refused(scores=s, edges=torch.tensor([0.0, 0.5, float("inf")]))
    assert "finite" in _refused(scores=s, edges=torch.tensor([0.0, float("nan"), 1.0]))
    assert "[-128, 128]" in _refused(scores=s, edges=torch.tensor([0.0, 129.0]), want_sums=True)
    assert "[-128, 128]" in _refused(scores=s, range=(-200.0, 0.0), want_sums=True)
    assert "2^31" in _refused(scores=torch.zeros(2, 1).expand(2, 1 << 31), per_image=True)
    assert "2^31" in _refused(scores=torch.zeros(2, 1).expand(2, 1 << 30), per_image=False)
    assert "65535" in _refused(scores=torch.zeros(1, 1).expand(65536, 2))
    assert "dict" in _refused(scores=s, out=[s])
    # aliased outputs
    c = torch.zeros(2, 1, 5, dtype=torch.int64)
    assert "shares memory" in _refused(scores=s, groups=g, edges=e, out={"counts": g.view(-1)[:10].view(2, 1, 5)})
    assert "shares memory" in _refused(scores=s, edges=e, want_sums=True, out={"counts": c, "sums": c})
    assert "gradient" in _refused(scores=s, out={"counts": torch.zeros(3, requires_grad=True)})
    # counts of the readers
    assert "rank" in _refused(counts=torch.zeros(2, 5, dtype=torch.int64), curves=True)
    assert "int64" in _refused(counts=torch.zeros(1, 2, 5), curves=True)
    assert "G = 2" in _refused(counts=torch.zeros(1, 3, 5, dtype=torch.int64), curves=True)
    assert "bins + 3" in _refused(counts=torch.zeros(1, 2, 3, dtype=torch.int64), curves=True)
    assert "bins + 3" in _refused(counts=torch.zeros(1, 2, 6, dtype=torch.int64), edges=e)
    assert "dense" in _refused(counts=torch.zeros(1, 2, 10, dtype=torch.int64)[:, :, ::2], curves=True)
    assert "group" in _refused(counts=c, edges=e, otsu_groups=[1])
    assert "group" in _refused(counts=c, edges=e, otsu_groups=[-1])
    assert "nothing" in _refused(counts=c, edges=e, otsu_groups=[])
    assert "fallback" in _refused(counts=c, edges=e, fallback=float("nan"))
    # thresholds
    assert "thresh" in _refused(scores=s, thresh="0.3")
    assert "thresh" in _refused(scores=s, thresh=torch.zeros(3))
    assert "float32" in _refused(scores=s, thresh=torch.zeros(2, dtype=torch.float64))
    # the confidence table
    z, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    assert "rank" in _refused(logits=z[0], labels=y)
    assert "classes" in _refused(logits=torch.zeros(1, 65, 2, 2), labels=torch.zeros(1, 2, 2, dtype=torch.int64))
    assert "labels" in _refused(logits=z, labels=y[:, :3])
    assert "int64" in _refused(logits=z, labels=y.int())
    assert "ignore_index" in _refused(logits=z, labels=y, ignore_index=1.5)
    # the place is checked LAST: a host call that is otherwise fine is refused for where its tensors live
    assert "device tensor" in _refused(scores=s, groups=g, edges=e)
    assert "device tensor" in _refused(counts=c, edges=e)
    assert "device tensor" in _refused(logits=z, labels=y)
    for call in (lambda: ops.score_histogram(s), lambda: ops.threshold_curves(torch.zeros(1, 2, 5, dtype=torch.int64)),
                 lambda: ops.otsu_threshold(c, e), lambda: ops.threshold_per_image(s, 0.3),
                 lambda: ops.confidence_histogram(z, y)):
        with pytest.raises(WsdlError, match="device tensor"):
            call()
    with pytest.raises(WsdlError, match="2\\^21"):
        ops.otsu_threshold(c, e, segment_pixels=(1 << 21) + 1)


def test_the_c_abi_refuses_the_limits_again():
    """The entry points check the table limits and a HOST copy of the edges before anything is launched: every call below returns
    an error without a device (the pointers are never followed)."""
    from weaklysuperviseddl_amd._lib import lib
    L = lib()
    buf = np.zeros(4096, dtype=np.int64)
    p = buf.ctypes.data
    ok = np.array([0.0, 0.5, 1.0], dtype=F)

    def hist(edges_host, B=1, HW=16, G=2, nb=2, per_image=1, sums=None):
        return L.wsdl_score_hist(p, None, p, None if edges_host is None else edges_host.ctypes.data, B, HW, G, nb, per_image, p + 1024, sums, None)
    big = np.arange(1027, dtype=F)
    for rc, why in ((hist(big, nb=1025), "bins"), (hist(ok, G=33), "groups"), (hist(big, G=4, nb=1024), "slots"), (hist(None), "edges_host"),
                    (hist(np.array([0, 1, 1], dtype=F)), "ascending"), (hist(np.array([0, 2, 1], dtype=F)), "ascending"),
                    (hist(np.array([0, 1, np.inf], dtype=F)), "finite"), (hist(np.array([0, np.nan, 1], dtype=F)), "finite"),
                    (hist(np.array([0, 1, 129], dtype=F), sums=p + 2048), "[-128, 128]"), (hist(ok, HW=1 << 31), "2^31"),
                    (hist(ok, B=2, HW=1 << 30, per_image=0), "2^31"), (hist(ok, B=0), "B ="), (hist(ok, B=65536), "B ="), (hist(ok, per_image=2), "per_image"),
                    (L.wsdl_confidence_hist(p, p, p, ok.ctypes.data, 1, 65, 2, 2, -100, 2, 0, p + 1024, None, None, None, None), "C ="),
                    (L.wsdl_confidence_hist(p, p, p, big.ctypes.data, 1, 2, 2, 2, -100, 1025, 0, p + 1024, None, None, None, None), "bins"),
                    (L.wsdl_hist_curves(p, 1, 0, p + 1024, None), "bins"), (L.wsdl_hist_curves(p, 1, 2, p, None), "overlaps"),
                    (L.wsdl_otsu(p, p, 1, 2, 2, 3, 0.5, (1 << 21) + 1, p + 512, p + 640, p + 768, None), "2^21"),
                    (L.wsdl_otsu(p, p, 1, 2, 2, 4, 0.5, 0, p + 512, p + 640, p + 768, None), "group mask"),
                    (L.wsdl_otsu(p, p, 1, 2, 2, 0, 0.5, 0, p + 512, p + 640, p + 768, None), "group mask"),
                    (L.wsdl_otsu(p, p, 1, 4, 1024, 1, 0.5, 0, p + 512, p + 640, p + 768, None), "table limits"),
                    (L.wsdl_threshold_images(p, p + 512, 0, 16, 1, p + 1024, None, None), "B ="),
                    (L.wsdl_threshold_images(p, p + 512, 1, 16, 2, p + 1024, None, None), "positive_only"),
                    (L.wsdl_threshold_images(p, p + 512, 1, 1 << 31, 1, p + 1024, None, None), "HW =")):
        assert rc != 0, why
    # (the message of the LAST refusal is readable; the loop above only looked at the codes)
    assert hist(np.array([0, 1, 1], dtype=F)) != 0 and b"ascending" in L.wsdl_last_error()
    assert L.wsdl_otsu(p, p, 1, 2, 2, 3, 0.5, (1 << 21) + 1, p + 512, p + 640, p + 768, None) != 0 and b"2^21" in L.wsdl_last_error()
