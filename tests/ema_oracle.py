"""numpy float64 oracles of the EMA teacher kernels (csrc/ema.hip) and the inputs the CPU and the GPU tests share.

The update: ``e <- e + a (p - e)``, ``a = 1 - d``, ``d = decay`` (the float32 value, widened) or with warm-up ``min(decay, float32((1 +
k) / (10 + k)))`` for the k-th update (0-based); ``a == 1`` is a copy.  ``ema_update`` carries ``e`` in float64, ``ema_update32`` rounds it to
float32 after every update, as the device stores it.  ``ema_update_fma`` is the same with an emulated fused multiply-add (error-free
product, then one sum): what the device evaluates.

Label correction: ``teacher_targets`` is a loop over pixels in Python floats (float64)."""
import math

import numpy as np


def decay_at(decay, warmup, k):
    """The decay of update k as the float32 it is on the device, widened: the warm-up ratio is rounded like the decay."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32((1.0 + k) / (10.0 + k)))
    return float(d)


def ema_update(e, p, decay, warmup, k):
    """float64 in, float64 out (not rounded)."""
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    a = 1.0 - decay_at(decay, warmup, k)
    if a == 1.0:
        return p.copy()
    return e + a * (p - e)


def ema_update32(e32, p, decay, warmup, k):
    return ema_update(np.asarray(e32, np.float32), p, decay, warmup, k).astype(np.float32)


def _two_prod(a, b):
    """a * b = x + y exactly (Veltkamp / Dekker), element-wise in float64."""
    x = a * b
    def split(v):
        c = 134217729.0 * v             # 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    y = al * bl - (((x - ah * bh) - al * bh) - ah * bl)
    return x, y


def fma_emulated(a, d, e):
    """``fma(a, d, e)`` of float64 arrays ``d``, ``e`` and a float ``a``: the product without rounding error, then one (two-sum
    compensated) addition.  Only ``+ - *`` of whole arrays: works on numpy arrays and on float64 torch tensors alike (every
    operation rounds by itself there too)."""
    x, y = _two_prod(d * 0.0 + a, d)
    s = x + e
    bb = s - x
    t = (x - (s - bb)) + (e - bb)       # x + e = s + t exactly
    return s + (t + y)


def ema_update_fma(e, p, decay, warmup, k):
    """The update as the device evaluates it, ``fma(a, p - e, e)`` - float64 in, float64 out."""
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    a = 1.0 - decay_at(decay, warmup, k)
    if a == 1.0:
        return p.copy()
    return fma_emulated(a, p - e, e)


def ulp_distance(a, b):
    """Distance in float32 units in the last place (ordered-integer difference); NaN against NaN and equal infinities are 0."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


FLAT_SIZES = (1, 3, 4, 5, 64, 1027, 4 * 256 * 3 + 2, 2 ** 23 + 1029)
DATA_KINDS = ("unit", "offset", "huge_e")
DECAYS = (0.0, 0.5, 0.999, 0.9999)
WARM_KS = (0, 1, 9, 1000)


def flat_data(n, kind, seed):
    """(e, p) float32 of n elements: at scale 1, at offset 100, or with |e| = 2^30 |p|."""
    rng = np.random.default_rng(seed)
    e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    if kind == "offset":
        e, p = e + np.float32(100.0), p + np.float32(100.0)
    elif kind == "huge_e":
        e = (np.abs(p) * np.float32(2.0 ** 30) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32)
    elif kind != "unit":
        raise ValueError(kind)
    return e, p


def flat_settings(n):
    """(decay, warmup, k) the flat kernel is run with at size n: the full cross product, thinned at the one large size (8.4 M
    elements) to six settings that still cover every decay, warm-up off, and every k with the warm-up on."""
    if n > 1 << 20:
        return [(0.0, False, 0), (0.5, True, 0), (0.5, True, 1), (0.9999, True, 9), (0.999, True, 1000), (0.9999, False, 0)]
    return [(d, True, k) for d in DECAYS for k in WARM_KS] + [(d, False, 0) for d in DECAYS]


# ---- label correction -------------------------------------------------------------------------------------------------------
def teacher_targets(logits, labels, tau, mode="replace", ignore_index=-100):
    """-> (labels', conf float32, counts (kept, changed, ignored), p float64 per pixel).  ``tau`` is compared as the float32 it is
    stored as, against the float32 ``p``."""
    logits, labels = np.asarray(logits, np.float32), np.asarray(labels, np.int64)
    B, C, H, W = logits.shape
    tau32 = np.float32(tau)
    out, conf, p64 = labels.copy(), np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.float64)
    counts = [0, 0, 0]
    for b in range(B):
        for y in range(H):
            for x in range(W):
                l = [float(v) for v in logits[b, :, y, x]]
                t = 0
                for c in range(1, C):
                    if l[c] > l[t]:
                        t = c
                finite = all(math.isfinite(v) for v in l)
                p = 1.0 / sum(math.exp(v - l[t]) for v in l) if finite else 0.0
                p64[b, y, x] = p
                lab = int(labels[b, y, x])
                if lab == ignore_index:
                    counts[2] += 1
                    continue
                p32 = np.float32(p)
                conf[b, y, x] = p32
                if finite and p32 >= tau32 and t != lab:
                    out[b, y, x] = t if mode == "replace" else ignore_index
                    counts[1] += 1
                else:
                    counts[0] += 1
    return out, conf, np.asarray(counts, np.int64), p64


def teacher_targets32(logits, labels, tau, mode="replace", ignore_index=-100):
    """The same contract evaluated in float32 (torch's softmax): -> (labels', counts)."""
    import torch
    lg = torch.from_numpy(np.asarray(logits, np.float32))
    lab = torch.from_numpy(np.asarray(labels, np.int64))
    finite = torch.isfinite(lg).all(dim=1)
    p = torch.softmax(torch.nan_to_num(lg, nan=0.0, posinf=0.0, neginf=0.0), dim=1).amax(dim=1)
    t = torch.from_numpy(np.nan_to_num(lg.numpy(), nan=-3e38, posinf=3e38, neginf=-3e38).argmax(axis=1))    # numpy: the first maximum
    ign = lab == ignore_index
    flip = finite & (p >= float(np.float32(tau))) & (t != lab) & ~ign
    out = torch.where(flip, t if mode == "replace" else torch.full_like(lab, ignore_index), lab)
    counts = np.asarray([int((~flip & ~ign).sum()), int(flip.sum()), int(ign.sum())], np.int64)
    return out.numpy(), counts


# the last three have H W % 4 == 0 - four pixels per lane - at C = 2, at C = 3 (channels in registers) and at C = 21 (two passes)
TEACHER_SHAPES = ((1, 2, 1, 1), (1, 2, 1, 7), (2, 3, 5, 7), (2, 21, 37, 53), (1, 64, 33, 65), (1, 2, 3, 300), (2, 3, 4, 6), (2, 21, 8, 10))
TEACHER_TAUS = (0.0, 0.6, 0.9, 1.5)
TEACHER_CONTENTS = ("mixed", "agree")
TAU_BAND = 2.0 ** -22


def teacher_case(shape, content, seed):
    """(logits float32, labels int64): logits whose per-pixel scale runs from 0 to 6, so that the softmax maximum straddles every
    tau in (1 / C, 1); planted ties of the two largest logits, NaN / +inf / -inf logits, gaps of +40 and -40; labels with ignored
    (-100) pixels ('mixed'), or equal to the teacher's class everywhere ('agree')."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal(shape) * rng.uniform(0.0, 6.0, (B, 1, H, W))).astype(np.float32)
    n = B * H * W
    flat = logits.transpose(0, 2, 3, 1).reshape(n, C)          # a copy: written back below
    pick = rng.permutation(n)
    def take(i):
        return pick[i % n] if n >= 8 or i < n else None
    for i, what in enumerate(("tie", "nan", "+inf", "-inf", "+40", "-40", "tie", "nan")):
        for rep in range(max(1, n // 64)):
            q = take(i + 8 * rep)
            if q is None:
                continue
            if what == "tie":
                flat[q, :] = np.float32(-1.5)
                flat[q, C - 1] = flat[q, 0] = np.float32(2.25)          # the first class wins
            elif what == "nan":
                flat[q, rng.integers(C)] = np.nan
            elif what == "+inf":
                flat[q, rng.integers(C)] = np.inf
            elif what == "-inf":
                flat[q, rng.integers(C)] = -np.inf
            elif what == "+40":
                flat[q, rng.integers(C)] += np.float32(40.0)
            else:
                flat[q, rng.integers(C)] -= np.float32(40.0)
    logits = flat.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()
    if content == "agree":
        safe = np.nan_to_num(logits, nan=-3e38, posinf=3e38, neginf=-3e38)
        labels = safe.argmax(axis=1).astype(np.int64)
    else:
        labels = rng.integers(0, C, (B, H, W)).astype(np.int64)
        labels[rng.random((B, H, W)) < 0.15] = -100
    return logits, labels
