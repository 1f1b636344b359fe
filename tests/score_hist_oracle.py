"""numpy oracle of the score-histogram ops (include/wsdl_hip.h "score histograms"): the slot rule, the fixed-point sums, the
confusion curves, Otsu's criterion and the host reductions.  tests/test_score_hist.py holds it to independent formulations."""
import numpy as np

SUM_SCALE = np.float32(16777216.0)


def uniform_edges(lo, hi, bins):
    return np.linspace(float(lo), float(hi), bins + 1, dtype=np.float64).astype(np.float32)


def slots(v, edges):
    """slot 0: v < e[0]; 1 + k: e[k] <= v < e[k+1]; nb + 1: v >= e[nb]; nb + 2: NaN."""
    v, edges = np.asarray(v, dtype=np.float32), np.asarray(edges, dtype=np.float32)
    s = np.searchsorted(edges, v, side="right").astype(np.int64)
    return np.where(np.isnan(v), edges.shape[0] + 1, s)


def fixed(v):
    """int64(v * 2^24): the float32 product is exact, the conversion truncates (finite v)."""
    return np.trunc(np.asarray(v, dtype=np.float32) * SUM_SCALE).astype(np.int64)


def histogram(scores, groups, edges, num_groups=1, per_image=True, want_sums=False):
    """scores (B, ...) float32, groups the same shape (int64) or None -> counts (S, G, nb + 3) int64 [, sums]."""
    scores = np.asarray(scores, dtype=np.float32)
    B = scores.shape[0]
    v = scores.reshape(B, -1)
    g = np.zeros(v.shape, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64).reshape(B, -1)
    nb = len(edges) - 1
    S = B if per_image else 1
    counts = np.zeros((S, num_groups, nb + 3), dtype=np.int64)
    sums = np.zeros_like(counts)
    for b in range(B):
        s = slots(v[b], edges)
        ok = (g[b] >= 0) & (g[b] < num_groups)
        flat = g[b][ok] * (nb + 3) + s[ok]
        seg = b if per_image else 0
        counts[seg] += np.bincount(flat, minlength=num_groups * (nb + 3)).reshape(num_groups, nb + 3)
        inside = ok & (s >= 1) & (s <= nb)
        fx = fixed(np.where(inside, v[b], 0))
        np.add.at(sums[seg].reshape(-1), (g[b] * (nb + 3) + s)[inside], fx[inside])
    return (counts, sums) if want_sums else counts


def curves(counts):
    """counts (S, 2, nb + 3) -> (S, nb + 1, 4) = TP FP FN TN of v >= edges[k]."""
    counts = np.asarray(counts, dtype=np.int64)
    neg, pos = counts[:, 0], counts[:, 1]
    suffix = lambda c: np.cumsum(c[:, 1:-1][:, ::-1], axis=1)[:, ::-1]          # noqa: E731  slots k + 1 .. nb + 1
    tp, fp = suffix(pos), suffix(neg)
    fn, tn = pos.sum(axis=1, keepdims=True) - tp, neg.sum(axis=1, keepdims=True) - fp
    return np.stack([tp, fp, fn, tn], axis=-1)


def otsu(counts, edges, groups=None, fallback=0.5):
    """Per segment (k*, threshold float32, q float64) by the header's formula in int64 / float64; k* = -1 and the fallback with
    fewer than two occupied bins."""
    counts = np.asarray(counts, dtype=np.int64)
    S, G, row = counts.shape
    nb = row - 3
    sel = list(range(G)) if groups is None else sorted(set(groups))
    ks, ts, qs = [], [], []
    for s in range(S):
        h = counts[s, sel, 1:nb + 1].sum(axis=0)
        i = np.arange(nb, dtype=np.int64)
        N, T = h.sum(), (i * h).sum()
        w0, s0 = np.cumsum(h)[:max(nb - 1, 0)], np.cumsum(i * h)[:max(nb - 1, 0)]
        w1, s1 = N - w0, T - s0
        D = s0 * w1 - s1 * w0
        ok = (w0 > 0) & (w1 > 0)
        if not ok.any():
            ks.append(-1), ts.append(np.float32(fallback)), qs.append(0.0)
            continue
        q = np.full(w0.shape, -1.0)
        q[ok] = (D[ok].astype(np.float64) * D[ok].astype(np.float64)) / (w0[ok] * w1[ok]).astype(np.float64)
        k = int(np.argmax(q))                                                   # the first maximum
        ks.append(k), ts.append(np.float32(edges[k + 1])), qs.append(float(q[k]))
    return np.array(ks, dtype=np.int32), np.array(ts, dtype=np.float32), np.array(qs, dtype=np.float64)


def threshold_images(scores, thresh, positive_only=True):
    scores = np.asarray(scores, dtype=np.float32)
    t = np.asarray(thresh, dtype=np.float32).reshape((-1,) + (1,) * (scores.ndim - 1))
    with np.errstate(invalid="ignore"):
        m = scores >= t
        if positive_only:
            m &= scores > 0
    return m.astype(np.uint8)


def confidence_planes(logits, dtype=np.float64):
    """(conf, pred): the softmax maximum evaluated in ``dtype`` (NaN where a logit is not finite) and the first arg-max."""
    z = np.asarray(logits).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        m = z.max(axis=1, keepdims=True)
        conf = (dtype(1) / np.exp(z - m).sum(axis=1, dtype=dtype)).astype(dtype)
    conf[~np.isfinite(np.asarray(logits)).all(axis=1)] = np.nan
    return conf, np.argmax(np.asarray(logits), axis=1).astype(np.int64)


def confidence_groups(pred, labels, ignore_index=-100):
    return np.where(labels == ignore_index, -1, (pred == labels).astype(np.int64))


# ---- the host reductions, by explicit loops
def iou_curve(cv, empty=1.0):
    cv = np.asarray(cv, dtype=np.float64)
    out = np.empty(cv.shape[:-1])
    for idx in np.ndindex(*out.shape):
        tp, fp, fn, _tn = cv[idx]
        out[idx] = tp / (tp + fp + fn) if tp + fp + fn > 0 else empty
    return out


def fbeta_curve(cv, beta2=0.3):
    cv = np.asarray(cv, dtype=np.float64)
    out = np.zeros(cv.shape[:-1])
    for idx in np.ndindex(*out.shape):
        tp, fp, fn, _tn = cv[idx]
        p = tp / (tp + fp) if tp + fp > 0 else 1.0
        r = tp / (tp + fn) if tp + fn > 0 else 0.0
        out[idx] = (1 + beta2) * p * r / (beta2 * p + r) if beta2 * p + r > 0 else 0.0
    return out


def pr(cv):
    cv = np.asarray(cv, dtype=np.float64).reshape(-1, np.shape(cv)[-2], 4).sum(axis=0)
    p = [tp / (tp + fp) if tp + fp > 0 else 1.0 for tp, fp, fn, tn in cv]
    r = [tp / (tp + fn) if tp + fn > 0 else 0.0 for tp, fp, fn, tn in cv]
    return np.array(p), np.array(r)


def average_precision(cv):
    p, r = pr(cv)
    return sum((r[k] - (r[k + 1] if k + 1 < len(r) else 0.0)) * p[k] for k in range(len(r)))


def mae(scores, target):
    """mean |clip(v) - target| over the non-NaN pixels of a map in [0, 1], from the float32 values' 2^-24 truncations"""
    v = np.asarray(scores, dtype=np.float32).reshape(-1)
    t = np.asarray(target).reshape(-1)
    ok = ~np.isnan(v)
    fx = fixed(np.clip(v[ok], 0, 1)).astype(np.float64) / float(SUM_SCALE)
    return float(np.abs(fx - t[ok]).sum() / ok.sum())


def ece(conf, correct, bins):
    """(ece, accuracy, confidence, count) per bin of [0, 1] in ``bins`` uniform bins, conf == 1 in the last one; NaN left out"""
    conf, correct = np.asarray(conf, dtype=np.float32).reshape(-1), np.asarray(correct).reshape(-1)
    s = slots(conf, uniform_edges(0, 1, bins))
    fx = fixed(np.where(np.isnan(conf), 0, conf)).astype(np.float64) / float(SUM_SCALE)
    acc, cf, cnt = np.full(bins, np.nan), np.full(bins, np.nan), np.zeros(bins, dtype=np.int64)
    total, e = 0, 0.0
    for k in range(bins):
        m = (s == k + 1) | ((s == bins + 1) if k == bins - 1 else False)
        cnt[k] = m.sum()
        if cnt[k]:
            acc[k], cf[k] = correct[m].mean(), fx[m].sum() / cnt[k]
            e += cnt[k] * abs(acc[k] - cf[k])
            total += cnt[k]
    return (e / total if total else 0.0), acc, cf, cnt


def tau_for_precision(conf, correct, edges, target):
    conf, correct = np.asarray(conf, dtype=np.float32).reshape(-1), np.asarray(correct).reshape(-1)
    for e in edges:
        with np.errstate(invalid="ignore"):
            m = conf >= e
        if m.any() and correct[m].mean() >= target:
            return float(e)
    return None
