"""CPU oracle of the boundary-path ops (include/wsdl_hip.h "IRN boundary paths"; Ahn, Cho & Kwak, CVPR 2019): vectorised torch
with a ``dtype`` argument - float64 is the reference, the same code in float32 the yardstick of the parity bound.

Pairs, validity, kinds and counts are those of tests/affinity_oracle.py.  The affinity of a pair is ``1 - max`` of the boundary
map over the pair's path; the maximum is ``torch.max(dim)`` over the stacked shifted slices of the path's points, so the
first-index tie rule and the NaN rule are torch's own.  The backward is an explicit scatter to the arg index (``index_add_``)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_oracle as ao  # noqa: E402

# (B, h, w)
CASES = (
    (1, 1, 1),             # no valid pair at all
    (1, 1, 7),
    (1, 7, 1),
    (2, 5, 7),             # at radius 8 every long offset leaves the image
    (1, 33, 65),           # tile seams and ragged edges
    (2, 64, 64),
    (1, 70, 70),
    (1, 3, 300),
)
RADII = (2, 5, 8)
CONTENTS = ("smooth", "quantised", "line")
WALK_STEPS = (1, 16, 256)


def paths(radius):
    """One list of (y, x) per offset of ``ao.offsets(radius)``: the integer points of the rectangle between (0,0) and the offset
    with (dy x - dx y)^2 < dy^2 + dx^2, in raster order."""
    out = []
    for dy, dx in ao.offsets(radius):
        out.append([(y, x) for y in range(0, dy + 1) for x in range(min(0, dx), max(0, dx) + 1)
                    if (dy * x - dx * y) ** 2 < dy * dy + dx * dx])
    return out


def make_edge(B, h, w, seed, content="smooth"):
    """A boundary map in [0, 1].  'smooth': random, neighbours related, strictly inside (0, 1); 'quantised': multiples of 1/8
    with 0 and 1 among them - ties on every path, valid pairs at exactly 0 and exactly 1; 'line': a one-pixel-wide line of 1
    (a column, and a row through it) on zeros."""
    g = torch.Generator().manual_seed(seed)
    if content == "line":
        e = torch.zeros(B, h, w)
        e[:, :, w // 2] = 1.0
        if h > 2:
            e[:, h // 3, :] = 1.0
        return e
    base = torch.rand(B, h, w, generator=g)
    if h > 1:
        base[:, 1:] = 0.5 * base[:, 1:] + 0.5 * base[:, :-1]
    if w > 1:
        base[:, :, 1:] = 0.5 * base[:, :, 1:] + 0.5 * base[:, :, :-1]
    if content == "quantised":
        return (torch.rand(B, h, w, generator=g) * 12 - 3).floor().clamp(0, 8) / 8      # (a third of the pixels at exactly 0)
    return base.clamp(1e-3, 1 - 1e-3).float()


def make_logits(B, h, w, seed):
    """The smooth map through ``logit``, clamped to +-6, with a few pixels at +-40."""
    z = torch.logit(make_edge(B, h, w, seed).double()).clamp(-6, 6).float()
    g = torch.Generator().manual_seed(seed + 1)
    flat = z.view(-1)
    n = flat.numel()
    for k in range(min(4, n)):
        flat[int(torch.randint(0, n, (1,), generator=g))] = 40.0 if k % 2 == 0 else -40.0
    return z


def path_max(edge, radius, dtype=torch.float64):
    """(max (B,P,h,w) in ``dtype``, arg (B,P,h,w) int64, valid (B,P,h,w) bool): the maximum over the path, first index on ties,
    NaN as torch.max has it; 0 / 0 at an invalid pair."""
    e = edge.to(dtype)
    B, h, w = e.shape
    offs, pts = ao.offsets(radius), paths(radius)
    m = torch.zeros(B, len(offs), h, w, dtype=dtype)
    arg = torch.zeros(B, len(offs), h, w, dtype=torch.int64)
    valid = torch.zeros(B, len(offs), h, w, dtype=torch.bool)
    for j, (dy, dx) in enumerate(offs):
        win = ao.window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, _, _ = win
        stack = torch.stack([e[:, ys.start + y:ys.stop + y, xs.start + x:xs.stop + x] for y, x in pts[j]], dim=0)
        val, idx = torch.max(stack, dim=0)
        m[:, j, ys, xs], arg[:, j, ys, xs], valid[:, j, ys, xs] = val, idx, True
    return m, arg, valid


def affinity(edge, radius, dtype=torch.float64):
    """(aff (B,P,h,w) in ``dtype``, arg int64): 1 - max over the path, 0 at an invalid pair."""
    m, arg, valid = path_max(edge, radius, dtype)
    return torch.where(valid, 1 - m, torch.zeros_like(m)), arg


def scatter_to_arg(values, arg, valid, radius):
    """(B,h,w): every valid pair's value added at the point of its path that ``arg`` names - the backward of the maximum."""
    B, P, h, w = values.shape
    out = torch.zeros(B, h * w, dtype=values.dtype)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    for j, pts in enumerate(paths(radius)):
        py = torch.tensor([p[0] for p in pts])
        px = torch.tensor([p[1] for p in pts])
        ok = valid[:, j]
        if not ok.any():
            continue
        ty = yy[None] + py[arg[:, j]]
        tx = xx[None] + px[arg[:, j]]
        target = (ty * w + tx)
        for b in range(B):
            out[b].index_add_(0, target[b][ok[b]], values[b, j][ok[b]])
    return out.view(B, h, w)


def affinity_backward(daff, arg, valid, radius):
    """dedge = - scatter of daff to the arg points."""
    return -scatter_to_arg(daff, arg, valid, radius)


def loss(logits, labels, radius, ignore_index=255, weights=(0.25, 0.25, 0.5), eps=1e-5, dtype=torch.float64):
    """(loss, dL/dlogits (B,h,w)) in ``dtype``: the count-normalised -log terms with sigmoid(-zmax) and sigmoid(zmax) formed
    separately, the pair coefficients scattered to the arg points."""
    zmax, arg, valid = path_max(logits, radius, dtype)
    kinds = ao.pair_kinds(labels, radius, ignore_index)
    n = ao.pair_counts(labels, radius, ignore_index).to(dtype)
    a, om = torch.sigmoid(-zmax), torch.sigmoid(zmax)
    s = [weights[k] / (n[k] + eps) for k in range(3)]
    k = kinds.to(dtype)
    pos, neg = -torch.log(a + eps), -torch.log(om + eps)
    L = s[0] * (pos * k[0]).sum() + s[1] * (pos * k[1]).sum() + s[2] * (neg * k[2]).sum()
    c = (s[0] * k[0] + s[1] * k[1]) * (a * om) / (a + eps) - s[2] * k[2] * (a * om) / (om + eps)
    return L, scatter_to_arg(c, arg, valid, radius)


def loss_autograd(logits, labels, radius, ignore_index=255, weights=(0.25, 0.25, 0.5), eps=1e-5):
    """The float64 loss written with ``amax`` and differentiated by torch: what ``loss`` is checked against on tie-free inputs."""
    z = logits.detach().double().requires_grad_()
    B, h, w = z.shape
    offs, pts = ao.offsets(radius), paths(radius)
    kinds = ao.pair_kinds(labels, radius, ignore_index)
    n = ao.pair_counts(labels, radius, ignore_index).double()
    L = z.sum() * 0
    for j, (dy, dx) in enumerate(offs):
        win = ao.window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, _, _ = win
        zmax = torch.stack([z[:, ys.start + y:ys.stop + y, xs.start + x:xs.stop + x] for y, x in pts[j]], dim=0).amax(dim=0)
        pos, neg = -torch.log(torch.sigmoid(-zmax) + eps), -torch.log(torch.sigmoid(zmax) + eps)
        for k in range(3):
            L = L + weights[k] / (n[k] + eps) * ((neg if k == 2 else pos) * kinds[k][:, j, ys, xs]).sum()
    L.backward()
    return L.detach(), z.grad


def edge_walk(edge, scores, radius, beta, steps, dtype=torch.float64):
    """{n: scores after n steps}: the stencil walk of tests/affinity_oracle.py under the path affinities, from the seed
    scores * (1 - edge)."""
    aff, _ = affinity(edge, radius, dtype)
    trans = ao.transitions(aff, beta, radius)
    seed = scores.to(dtype) * (1 - edge.to(dtype))[:, None]
    return ao.walk(trans, seed, steps, radius)
