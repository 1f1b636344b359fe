"""Oracle of the signed distance maps, the boundary loss (Kervadec et al., MIDL 2019) with its gradient, and the surface
distance statistics behind Hausdorff / HD95 / ASSD (include/wsdl_hip.h "signed-distance boundary loss, surface distances"),
written from the contract on the brute-force transforms of tests/edt_oracle.py.

``phi``, the loss and the gradient exist in float64 and in float32: the float32 run - every operation in torch float32 on the
CPU, from the float32 logits and the float32 ``phi`` - against the float64 run is the yardstick of the device tests.  The
gradient is written out (``s_c (Phi_c - sum_j s_j Phi_j) scale / (K N)``), not taken from autograd; tests/test_boundary_loss.py
compares it with autograd.  Surfaces are defined WITHOUT distances, by the 4-neighbour rule; the distance between two
surfaces is the brute-force transform of the surface map."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import edt_oracle as eo

FAR = eo.FAR

# (B, H, W) of the device tests: a single pixel; a vector tail; odd strides; more than one workgroup of partials (1961 and
# 4096 pixels per image: 16 and 8 workgroups of 256 one- and four-pixel items); 96 x 130 - H W a multiple of 4, W not; a row
# wider than a workgroup
CASES = ((1, 1, 1), (1, 1, 7), (2, 5, 7), (3, 37, 53), (2, 64, 64), (2, 96, 130), (1, 3, 300))
CHANNELS = (2, 3, 21)
CLASS_LISTS = ((1,), (0, 1), (2, 0))


def dist2_separable(labels, value=1):
    """``eo.dist2(labels, value, "euclid", False)`` by brute force along one axis at a time - exact integer arithmetic, H + W
    candidates per pixel instead of H W: g[y, x] = the vertical distance to the nearest site of column x, then d2[y, x] = min
    over x' of g[y, x']^2 + (x - x')^2.  For the cases where the all-pairs oracle takes seconds; tests/test_boundary_loss.py
    shows the two equal."""
    inside = labels.to(torch.int64) == int(value)
    B, H, W = inside.shape
    none = 1 << 15                                                       # "no site in this column"; none^2 == FAR
    dy = (torch.arange(H)[:, None] - torch.arange(H)[None, :]).abs()
    dx2 = (torch.arange(W)[:, None] - torch.arange(W)[None, :]) ** 2
    out = []
    for sites in (~inside, inside):
        g = torch.where(sites[:, None, :, :], dy[None, :, :, None], none).min(dim=2).values          # (B,H,W)
        cand = torch.where(g[:, :, None, :] < none, g[:, :, None, :] ** 2 + dx2[None, None], FAR)   # (B,H,W,W')
        out.append(cand.min(dim=3).values)
    return out[0], out[1]


def signed_distance(labels, value=1, dtype=torch.float64, planes=None):
    """(B,H,W) in ``dtype``: +sqrt(d2_in) on OUT pixels, -(sqrt(d2_out) - 1) on IN pixels, computed in float64 and rounded
    once; 0 for a whole image whose class is absent or fills it.  ``planes``: ``eo.dist2(labels, value)`` when the caller
    has it already."""
    d_out, d_in = eo.dist2(labels, value, "euclid", False) if planes is None else planes
    inside = labels.to(torch.int64) == int(value)
    phi = torch.where(inside, 1.0 - d_out.double().sqrt(), d_in.double().sqrt())
    flat = ((d_out >= FAR) | (d_in >= FAR)).flatten(1).any(dim=1)
    phi[flat] = 0.0
    return phi.to(dtype)


def signed_distance_classes(labels, classes, dtype=torch.float64):
    return torch.stack([signed_distance(labels, c, dtype) for c in classes], dim=1)


def loss_and_grad(logits, phi, labels=None, classes=(1,), ignore_index=-100, scale=1.0, dtype=torch.float64):
    """(loss, grad) in ``dtype``: loss = scale / (K N) sum over valid p, c of s_c Phi_c; grad = d loss / d logits, written
    out.  ``phi`` (B,K,H,W); N == 0 gives zeros."""
    z, phi = logits.to(dtype), phi.to(dtype)
    B, C, H, W = z.shape
    K = len(classes)
    s = torch.softmax(z, dim=1)
    big = torch.zeros_like(z)
    for k, c in enumerate(classes):
        big[:, c] = phi[:, k]
    valid = torch.ones(B, H, W, dtype=torch.bool) if labels is None else labels != ignore_index
    n = int(valid.sum())
    if n == 0:
        return torch.zeros((), dtype=dtype), torch.zeros_like(z)
    v = valid.to(dtype)
    dot = (s * big).sum(dim=1)
    f = torch.tensor(scale, dtype=dtype) / torch.tensor(float(K * n), dtype=dtype)
    loss = (dot * v).sum() * f
    grad = s * (big - dot[:, None]) * v[:, None] * f
    return loss, grad


# ------------------------------------------------------------------------------------------------ surface distances
def surface(mask):
    """bool (B,H,W) -> the pixels of the mask with a 4-neighbour outside the mask or outside the image."""
    m = F.pad(mask.to(torch.bool), (1, 1, 1, 1), value=False)
    inner = m[:, 1:-1, 1:-1] & m[:, :-2, 1:-1] & m[:, 2:, 1:-1] & m[:, 1:-1, :-2] & m[:, 1:-1, 2:]
    return mask.to(torch.bool) & ~inner


def directed_d2(surf_from, surf_to):
    """Per image: the int64 squared distances from every pixel of ``surf_from`` to the nearest pixel of ``surf_to`` (FAR when
    ``surf_to`` is empty), in raster order."""
    _, to = eo.dist2(surf_to.to(torch.int64), 1, "euclid", False)
    return [to[b][surf_from[b]] for b in range(surf_from.shape[0])]


def rank(n, percentile):
    """The rank from the largest of the nearest-rank percentile: min(n, 1 + floor((1 - percentile / 100) n)), the product in
    double - the rank rule of wsdl_kth_value with k = 1, frac = 1 - percentile / 100."""
    frac = 1.0 - percentile / 100.0
    return int(min(n, 1 + int(np.floor(np.float64(frac) * np.float64(n)))))


def nearest_rank(d2, percentile):
    """The ``rank``-th largest of a 1-D int64 tensor as a float; +inf for an empty one."""
    n = int(d2.numel())
    if n == 0:
        return math.inf
    return float(torch.sort(d2, descending=True).values[rank(n, percentile) - 1])


def surface_stats(preds, labels, value=1, percentile=95.0):
    """dict of numpy arrays (B,2): n (int64), max_d2 (int64), sum_d (float64, math.fsum: the correctly rounded sum), pct_d2
    (float64).  Index 0: pred -> gt, 1: gt -> pred."""
    sa, sb = surface(preds.to(torch.int64) == value), surface(labels.to(torch.int64) == value)
    sets = list(zip(directed_d2(sa, sb), directed_d2(sb, sa)))
    out = {"n": [], "max_d2": [], "sum_d": [], "pct_d2": []}
    for pair in sets:
        out["n"].append([int(d.numel()) for d in pair])
        out["max_d2"].append([int(d.max()) if d.numel() else 0 for d in pair])
        out["sum_d"].append([math.fsum(math.sqrt(v) for v in d.tolist()) for d in pair])
        out["pct_d2"].append([nearest_rank(d, percentile) for d in pair])
    return {"n": np.array(out["n"], dtype=np.int64), "max_d2": np.array(out["max_d2"], dtype=np.int64),
            "sum_d": np.array(out["sum_d"], dtype=np.float64), "pct_d2": np.array(out["pct_d2"], dtype=np.float64)}


def metrics(stats):
    """(per_image, means, n_defined) from ``surface_stats``, written from the definitions: hd = the larger directed maximum,
    hd95 = the larger directed percentile, assd = the pooled mean; nan where a surface is empty; means over the rest."""
    per = []
    for n, mx, sm, pc in zip(stats["n"], stats["max_d2"], stats["sum_d"], stats["pct_d2"]):
        if min(n) == 0:
            per.append({"hd": math.nan, "hd95": math.nan, "assd": math.nan})
        else:
            per.append({"hd": math.sqrt(max(mx)), "hd95": math.sqrt(max(pc)), "assd": (sm[0] + sm[1]) / float(n[0] + n[1])})
    ok = [p for p in per if not math.isnan(p["hd"])]
    means = {}
    for key in ("hd", "hd95", "assd"):
        acc = 0.0
        for p in ok:
            acc += p[key]
        means[key] = acc / len(ok) if ok else math.nan
    return per, means, len(ok)


def make_logits(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(B, C, H, W, generator=g)).contiguous()
