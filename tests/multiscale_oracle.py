"""CPU oracle of the multi-scale + flip fusion (include/wsdl_hip.h "multi-scale fusion"), written from the contract in torch: a
``dtype`` argument runs it in float64 (the reference) or in float32 with the device's operation order (the yardstick of the
parity bound: resampling and ``exp`` in float32, the members combined in double and rounded once).  Nothing here comes from
the reference project, which has no such step."""
import functools

import torch

TARGETS = ((1, 1), (1, 7), (7, 1), (5, 7), (37, 53), (64, 64), (96, 130), (3, 300))
CHANNELS = (1, 2, 3, 21, 64)
WIDE_FROM = 5           # TARGETS[5:] are the wide ones: they carry 1, 2 or 3 channels (geometries)
COMBOS = tuple((a, r, w) for a in ("none", "softmax", "sigmoid") for r, w in (("mean", False), ("mean", True), ("max", False)))


def lerp(n_out, n_in, dtype):
    """ATen's align_corners=False source index and weights of one axis: (i0, i1, l0, l1)."""
    scale = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    s = (scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = s - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def resize(x, size, dtype):
    """bilinear_at of csrc/bilinear.h on (N,C,h,w): rows first (two taps each), then the two rows.  The input's own size: itself."""
    H, W = size
    x = x.to(dtype)
    if tuple(x.shape[-2:]) == (H, W):
        return x
    y0, y1, ly0, ly1 = lerp(H, x.shape[-2], dtype)
    x0, x1, lx0, lx1 = lerp(W, x.shape[-1], dtype)
    top = lx0 * x[..., y0, :][..., x0] + lx1 * x[..., y0, :][..., x1]
    bot = lx0 * x[..., y1, :][..., x0] + lx1 * x[..., y1, :][..., x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def scale_flip(x, size, flip, dtype=torch.float32):
    r = resize(x, size, dtype)
    return torch.cat([r, r.flip(-1)]) if flip else r


def members(sources, size, mirrored, dtype):
    """The resized members in order - a source's plain half, then its mirrored half un-mirrored - and the source index of each."""
    if isinstance(mirrored, bool):
        mirrored = [mirrored] * len(sources)
    out, owner = [], []
    for k, (src, m) in enumerate(zip(sources, mirrored)):
        r = resize(src, size, dtype)
        if m:
            B = r.shape[0] // 2
            out += [r[:B], r[B:].flip(-1)]
            owner += [k, k]
        else:
            out.append(r)
            owner.append(k)
    return out, owner


def activate(v, activation, dtype):
    """A member's values (B,C,H,W) in ``dtype`` -> float64 contributions: the exponential in ``dtype``, the rest in double."""
    if activation == "none":
        return v.double()
    if activation == "softmax":
        e = (v - v.amax(dim=1, keepdim=True)).exp()
        return e.double() * (1.0 / e.double().sum(dim=1, keepdim=True))
    if activation == "sigmoid":
        e = (-v.abs()).exp().double()
        return torch.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    raise ValueError(activation)


def fuse_members(mem, owner, weights, activation, reduce, dtype):
    if reduce == "mean":
        weights = [1.0] * (max(owner) + 1) if weights is None else [float(w) for w in weights]
        total = sum(weights[k] for k in owner)
        acc = torch.zeros(mem[0].shape, dtype=torch.float64)
        for v, k in zip(mem, owner):
            if weights[k] != 0.0:
                acc = acc + (weights[k] / total) * activate(v, activation, dtype)
    else:
        acc = activate(mem[0], activation, dtype)
        for v in mem[1:]:
            acc = torch.maximum(acc, activate(v, activation, dtype))       # NaN propagates
    return acc.to(dtype)


def fuse(sources, size, mirrored=False, weights=None, activation="none", reduce="mean", dtype=torch.float64):
    mem, owner = members(sources, size, mirrored, dtype)
    return fuse_members(mem, owner, weights, activation, reduce, dtype)


def labels(scores, thresh=0.5, min_conf=0.0, ignore_index=255):
    """wsdl_pamr_labels' rule: (labels int64 (B,H,W), conf)."""
    if scores.shape[1] == 1:
        return (scores[:, 0] >= thresh).long(), scores[:, 0]
    best = scores[:, 0].clone()
    arg = torch.zeros(best.shape, dtype=torch.int64)
    for c in range(1, scores.shape[1]):
        better = scores[:, c] > best
        best = torch.where(better, scores[:, c], best)
        arg = torch.where(better, torch.full_like(arg, c), arg)
    return torch.where(best < min_conf, torch.full_like(arg, ignore_index), arg), best


def label_margin(scores, thresh=0.5, min_conf=0.0):
    """How far each pixel of float64 scores is from another label: the top-two gap (C = 1: the distance to thresh), and the
    distance of the maximum to min_conf where that is in use."""
    if scores.shape[1] == 1:
        return (scores[:, 0] - thresh).abs()
    top = scores.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    return torch.minimum(gap, (top[:, 0] - min_conf).abs()) if min_conf > 0 else gap


def max_normalize(x, thresh=None):
    """float32 (B, ...) -> v / max per image in double, rounded once; an image whose maximum is <= 0 or not finite stays."""
    out = x.clone()
    for b in range(x.shape[0]):
        m = x[b].max()          # a NaN anywhere makes it NaN
        if torch.isfinite(m) and m > 0:
            out[b] = (x[b].double() / m.double()).float()
    if thresh is None:
        return out
    return out, ((out >= thresh) & (out > 0)).to(torch.uint8)


def label_combos(C):
    """The combinations whose LABELS are compared with the float64 oracle's: those a caller takes labels from - the mean over
    scales and mirror images of softmax probabilities or of logits (C >= 2), of sigmoid probabilities or of raw maps against the
    threshold (C = 1).  A maximum over members keeps the worst member's coordinate rounding instead of averaging it (its
    yardstick is about three times the mean's) and no caller takes labels from one; the arg-max over per-class sigmoids, which
    saturate at 1, has top-two gaps at 64 classes below what float32 inputs resolve.  The SCORES of every combination are
    checked against the bound; the device's labels equal ``pamr_labels`` of its scores for every combination."""
    acts = ("none", "sigmoid") if C == 1 else ("none", "softmax")
    return tuple((a, "mean", w) for a in acts for w in (False, True))


def source_sizes(H, W):
    """1 x 1, smaller than the target, the target itself, larger than it."""
    return [(1, 1), ((H + 1) // 2, (W + 2) // 3), (H, W), (H + 3, W + (W + 2) // 3)]


def geometries():
    """(target, source sizes, mirrored flags, B, C): every target with 1, 2 and 4 sources; the channel counts, batch sizes,
    mirrored patterns and the pick of source sizes rotate so that every value meets every target."""
    out = []
    for t, (H, W) in enumerate(TARGETS):
        pool = source_sizes(H, W)
        for j, n in enumerate((1, 2, 4)):
            k = 3 * t + j
            sizes = [pool[(k + i) % 4] for i in range(n)]
            mirrored = [bool((t // 2 + j + i) % 2) for i in range(n)]
            C = CHANNELS[k % 5] if t < WIDE_FROM else CHANNELS[k % 3]
            out.append(((H, W), tuple(sizes), tuple(mirrored), (1, 3)[(t + j) % 2], C))
    return out


GEOMETRIES = geometries()


def make_sources(case):
    """Normal logits with standard deviation 2, seeded by the case."""
    (H, W), sizes, mirrored, B, C = GEOMETRIES[case]
    g = torch.Generator().manual_seed(1000 + case)
    return [torch.randn((2 * B if m else B), C, h, w, generator=g) * 2.0 for (h, w), m in zip(sizes, mirrored)]


def case_weights(case):
    n = len(GEOMETRIES[case][1])
    return [0.5 + ((case + 3 * i) % 4) * 0.75 for i in range(n)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per combination of the case: the float64 oracle, the float32 yardstick max |float32 oracle - float64 oracle| and the
    float32 oracle itself.  Computed once, shared, never written."""
    (H, W), _sizes, mirrored, _B, C = GEOMETRIES[case]
    srcs = make_sources(case)
    mem64, owner = members(srcs, (H, W), list(mirrored), torch.float64)
    mem32, _ = members(srcs, (H, W), list(mirrored), torch.float32)
    out = {}
    for act, red, weighted in COMBOS:
        if act == "softmax" and C == 1:
            continue
        w = case_weights(case) if weighted else None
        r64 = fuse_members(mem64, owner, w, act, red, torch.float64)
        r32 = fuse_members(mem32, owner, w, act, red, torch.float32)
        assert r32.dtype == torch.float32 and r64.dtype == torch.float64
        out[(act, red, weighted)] = dict(r64=r64, r32=r32, yard=(r32.double() - r64).abs().max().item())
    return dict(sources=srcs, combos=out)


def fused_coordinate_term(case, activation):
    """The derived extra term of the device bound, (B,C,1,1) or (B,1,1,1) - see tests/test_hip_multiscale.py.  The device forms
    the source coordinate with one rounding (``wsdl_bilinear_fwd``'s fused multiply-add, whose bits the contract demands), so below
    1/2 - everywhere on a one-pixel axis, at the first output pixels otherwise - ``l1`` has more than 24 bits and ``l0 = 1 - l1``
    is rounded: ``l0 + l1 = 1 + d``, ``|d| <= 2^-25`` per axis.  This oracle's unfused coordinate keeps ``l0 + l1 = 1`` exactly,
    and on equal taps (a 1 x 1 source, a clamped border) its two rounded products then sum to within half an ulp of the tap and
    round back to it: it is EXACT there, its yardstick 0, while the device's ``v (1 + d)`` plus the same product roundings may
    land one ulp off at each of the two lerp levels, and the second level's own roundings add less than one more: 3 ulp of the
    largest tap magnitude ``A`` of the plane, ``3 * 2^-23 A``.  Through an activation it shrinks by the activation's Lipschitz
    constant (sigmoid 1/4; softmax: sum_c |dp_k / dv_c| = 2 p_k (1 - p_k) <= 1/2, with the largest A over the channels); a
    weighted mean or a maximum over members does not enlarge it."""
    _target, _sizes, mirrored, B, _C = GEOMETRIES[case]
    A = None
    for src, m in zip(make_sources(case), mirrored):
        a = src.abs().double().amax(dim=(2, 3))                 # (B or 2B, C)
        a = torch.maximum(a[:B], a[B:]) if m else a
        A = a if A is None else torch.maximum(A, a)
    eps = 3.0 * 2.0 ** -23 * A
    if activation == "softmax":
        return 0.5 * eps.amax(dim=1, keepdim=True)[:, :, None, None]
    return (0.25 if activation == "sigmoid" else 1.0) * eps[:, :, None, None]


def bound(r64, yard, extra=0.0):
    """The project's standing bound, per element: max(4 x the float32 oracle's worst error of the case, 2^-23 |value|), plus a
    derived extra term where a test states one."""
    return torch.clamp(r64.abs() * 2.0 ** -23, min=4.0 * yard) + extra
