"""float64 restatement (numpy) of ``ops.cross_entropy_mined`` and an exact ``ops.kth_value``.

For pixel i with label y, logits z, v_i = [y != ignore_index and p_i != 0] (p: the pixel weight, default 1):

    nll_i = -log softmax(z_i)[y]                         the ranking statistic: no class weights, no smoothing
    per scope segment (the batch, or each image) with n = sum v:
      hard: K = min(n, min_kept (x B for scope 'batch')),  tau = K-th largest nll over v  (+inf for K = 0)
            kept_i = v_i and nll_i >= min(tau, -log(thresh))            (thresh None: the cap is +inf)
      trim: K = min(n, 1 + floor(drop_frac n)),            tau = K-th largest nll over v
            kept_i = v_i and nll_i <= tau
    m_i = kept_i p_i; the result is the weighted cross entropy of tests/weighted_ce_oracle.py with pixel weight m, restated
    here: l_i = m_i [(1-e) w[y] nll_i + (e/C) sum_c w[c] (-log s[c])], 'mean' divides by sum_i m_i w[y_i].

Ties at tau are all kept (inclusive).  tests/test_pixel_mining.py pins this against a torch float64 formulation.
"""
import numpy as np


def rank(n, k_abs, frac):
    """min(n, k_abs + floor(frac n)), the product in double as the kernel computes it."""
    return int(min(n, k_abs + int(np.floor(np.float64(frac) * np.float64(n)))))


def kth_value_exact(x, k_abs=0, frac=0.0, largest=True, valid=None):
    """(value, n) for ONE segment: the candidates are the non-NaN elements of ``x`` (any float dtype, kept as it is) marked
    in ``valid``; the value is an element of ``x`` found with np.partition."""
    x = np.asarray(x).reshape(-1)
    keep = ~np.isnan(x)
    if valid is not None:
        keep &= np.asarray(valid).reshape(-1) != 0
    c = x[keep]
    n = int(c.size)
    K = rank(n, k_abs, frac)
    if K == 0:
        return x.dtype.type(np.inf if largest else -np.inf), n
    idx = n - K if largest else K - 1
    return np.partition(c, idx)[idx], n


def log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def mined_ce(logits, labels, ignore_index=-100, mode="hard", thresh=None, min_kept=0, drop_frac=0.0, scope="batch", weight=None,
             label_smoothing=0.0, pixel_weight=None, reduction="mean", upstream=1.0):
    """dict(loss, grad, nll, valid, threshold, kept, n_valid, selection) in float64.  logits (B,C,H,W), labels (B,H,W) int,
    every label ``ignore_index`` or in [0, C)."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels).astype(np.int64)
    B, C, H, W = z.shape
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    p = np.ones((B, H, W)) if pixel_weight is None else np.asarray(pixel_weight, dtype=np.float64)
    e = float(label_smoothing)
    v = (y != ignore_index) & (p != 0)
    ys = np.where(v, y, 0)
    logs = log_softmax(z)
    nll = -np.take_along_axis(logs, ys[:, None], axis=1)[:, 0]
    nll = np.where(y != ignore_index, nll, 0.0)         # (what reduction='none' holds at an ignored pixel; never a candidate)
    S = B if scope == "image" else 1
    nl, vv = nll.reshape(S, -1), v.reshape(S, -1)
    kept = np.zeros_like(vv)
    tau, n_valid = np.zeros(S), np.zeros(S, dtype=np.int64)
    for s in range(S):
        if mode == "hard":
            tau[s], n_valid[s] = kth_value_exact(nl[s], min_kept * (B if scope == "batch" else 1), 0.0, True, vv[s])
            cap = np.inf if thresh is None else -np.log(np.float64(thresh))
            kept[s] = vv[s] & (nl[s] >= min(tau[s], cap))
        elif mode == "trim":
            tau[s], n_valid[s] = kth_value_exact(nl[s], 1, drop_frac, True, vv[s])
            kept[s] = vv[s] & (nl[s] <= tau[s])
        else:
            raise ValueError(mode)
    m = kept.reshape(B, H, W) * p
    wy = w[ys]
    wv = w.reshape(1, C, 1, 1)
    smooth = -(wv * logs).sum(axis=1)
    pix = m * ((1 - e) * wy * nll + (e / C) * smooth)
    A = (1 - e) * wy + (e / C) * w.sum()
    onehot = (np.arange(C).reshape(1, C, 1, 1) == ys[:, None]).astype(np.float64)
    grad = m[:, None] * (np.exp(logs) * A[:, None] - (1 - e) * wy[:, None] * onehot - (e / C) * wv)
    if reduction == "sum":
        loss, grad = pix.sum(), grad * upstream
    elif reduction == "mean":
        den = (m * wy).sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            loss = pix.sum() / den
            grad = np.where(m[:, None] != 0, grad * (upstream / den), 0.0)       # nothing kept: NaN loss, a gradient of zeros
    else:
        raise ValueError(reduction)
    return dict(loss=loss, grad=grad, nll=nll, valid=v, threshold=tau, kept=kept.sum(axis=1).astype(np.int64), n_valid=n_valid,
                selection=m)


def boundary_gaps(res, mode, thresh, min_kept, drop_frac, scope):
    """The smallest relative float64 distances that decide the selection of an oracle result ``res``: (between the last kept
    and the first dropped rank, between any candidate's nll and -log(thresh)).  inf where there is no such boundary."""
    B = res["nll"].shape[0]
    S = B if scope == "image" else 1
    nl, vv = res["nll"].reshape(S, -1), res["valid"].reshape(S, -1)
    g_rank, g_cap = np.inf, np.inf
    for s in range(S):
        c = np.sort(nl[s][vv[s]])[::-1]                 # descending
        n = c.size
        k = rank(n, min_kept * (B if scope == "batch" else 1), 0.0) if mode == "hard" else rank(n, 0, drop_frac)
        if 1 <= k < n:                                  # ranks k and k + 1 (1-based, from the largest)
            a, b = c[k - 1], c[k]
            g_rank = min(g_rank, abs(a - b) / max(abs(a), abs(b), 1e-300))
        if mode == "hard" and thresh is not None and n:
            cap = -np.log(np.float64(thresh))
            g_cap = min(g_cap, (np.abs(c - cap) / np.maximum(np.maximum(np.abs(c), cap), 1e-300)).min())
    return g_rank, g_cap
