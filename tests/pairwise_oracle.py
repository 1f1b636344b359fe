"""An independent second formulation of the pairwise-affinity losses (oracle/losses.py: ``pairwise_affinity_loss``,
``compute_affinities``, ``_affinity_stack``): a per-pixel loop in numpy float64 with explicit reflect indices - no ``F.pad``, no
stacked shifted views, no autograd.  For the K = w*w - 1 offsets o = (dy, dx) of a w x w window, dy major, centre skipped,

    a_k(q) = exp(-|I(q) - I(r(q + o))|^2 / (2 sc^2)  [- |o|^2 / (2 ss^2)]),    r(i) = -i (i < 0), 2 (n - 1) - i (i >= n), i

    normalise 0:  loss    = sum_{b,q,k,c} a_k(q) (P_c(q) - P_c(r(q + o)))^2 / (B H W K C)
    normalise 1:  loss[b] = sum_{q,k,c}   a_k(q) (P_c(q) - P_c(r(q + o)))^2 / (H W K)

TEST INFRASTRUCTURE ONLY.  tests/test_pairwise_oracle.py holds the torch oracle to this loop in float64;
tests/test_hip_pairwise_loss.py holds the device to the torch oracle and, for the affinity cache, to this loop."""
import math

import numpy as np
import torch


def reflect(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def offsets(window):
    """The K offsets in dy-major order, centre skipped."""
    r = window // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]


def forward_offsets(window):
    """The K/2 offsets of the affinity cache: (dy == 0, dx > 0), then dy > 0, in raster order."""
    return [(dy, dx) for dy, dx in offsets(window) if dy > 0 or (dy == 0 and dx > 0)]


def _np(t):
    return np.asarray(t.detach().cpu().double().numpy() if torch.is_tensor(t) else t, dtype=np.float64)


def _space(sigma_space):
    return sigma_space is not None and sigma_space > 0


def affinities(image, window, sigma_color, sigma_space=None):
    """(B,3,H,W) -> (K,B,H,W) float64, pixel by pixel."""
    img = _np(image)
    B, _, H, W = img.shape
    offs = offsets(window)
    out = np.zeros((len(offs), B, H, W))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                for k, (dy, dx) in enumerate(offs):
                    d = img[b, :, y, x] - img[b, :, reflect(y + dy, H), reflect(x + dx, W)]
                    e = -(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / (2.0 * sigma_color * sigma_color)
                    if _space(sigma_space):
                        e -= (dy * dy + dx * dx) / (2.0 * sigma_space * sigma_space)
                    out[k, b, y, x] = math.exp(e)
    return out


def softmax(preds):
    p = _np(preds)
    e = np.exp(p - p.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def loss(preds, image, window, sigma_color, sigma_space=None, apply_softmax=True, normalise=0, aff=None):
    """The loss of the loop formulation: a float (normalise 0) or a (B,) array (normalise 1).  ``aff``: ``affinities(...)`` of
    the same image, when many predictions are evaluated on it (central differences).  The terms of an image are added
    with ``math.fsum``, so that differences of two evaluations carry no summation noise."""
    P = softmax(preds) if apply_softmax else _np(preds)
    B, C, H, W = P.shape
    offs = offsets(window)
    a = affinities(image, window, sigma_color, sigma_space) if aff is None else aff
    per_image = []
    for b in range(B):
        terms = []
        for y in range(H):
            for x in range(W):
                for k, (dy, dx) in enumerate(offs):
                    d = P[b, :, y, x] - P[b, :, reflect(y + dy, H), reflect(x + dx, W)]
                    terms.append(a[k, b, y, x] * float(np.dot(d, d)))
        per_image.append(math.fsum(terms))
    K = len(offs)
    if normalise == 0:
        return math.fsum(per_image) / (B * H * W) / (K * C)
    return np.array(per_image) / (H * W) / K


def central_difference_gradient(preds, image, window, sigma_color, sigma_space, apply_softmax, normalise, weights=None, h=1e-6):
    """d (sum_b weights[b] loss[b]) / d preds by central differences of ``loss`` (float64, step ``h``)."""
    p = _np(preds).copy()
    a = affinities(image, window, sigma_color, sigma_space)
    w = None if weights is None else _np(weights)

    def value(q):
        v = loss(q, image, window, sigma_color, sigma_space, apply_softmax, normalise, aff=a)
        return float(v) if normalise == 0 else float(np.dot(v, w if w is not None else np.ones_like(v)))
    g = np.zeros_like(p)
    for idx in np.ndindex(*p.shape):
        keep = p[idx]
        p[idx] = keep + h
        up = value(p)
        p[idx] = keep - h
        down = value(p)
        p[idx] = keep
        g[idx] = (up - down) / (2.0 * h)
    return g


def forward_half_cache(image, window, sigma_color):
    """The colour affinities of the forward half of the window in the layout of ``ops.pairwise_cache``: cache[k][b][y][x] for
    the K/2 offsets of ``forward_offsets``; exactly 0 where the partner q + o lies outside the image (no reflection)."""
    img = _np(image)
    B, _, H, W = img.shape
    offs = forward_offsets(window)
    out = np.zeros((len(offs), B, H, W))
    for k, (dy, dx) in enumerate(offs):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    py, px = y + dy, x + dx
                    if 0 <= py < H and 0 <= px < W:
                        d = img[b, :, y, x] - img[b, :, py, px]
                        out[k, b, y, x] = math.exp(-(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / (2.0 * sigma_color * sigma_color))
    return out


def forward_half_of_stack(stack, window):
    """The same table cut out of the torch oracle's (K,B,H,W) colour-only affinity stack (any dtype): the yardstick of the
    cache in float32.  Where the partner is inside the image no reflection took part, so the stack's value is the pair's."""
    K, B, H, W = stack.shape
    full = offsets(window)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    maps = []
    for dy, dx in forward_offsets(window):
        inside = (yy + dy >= 0) & (yy + dy < H) & (xx + dx >= 0) & (xx + dx < W)
        maps.append(torch.where(inside, stack[full.index((dy, dx))], torch.zeros((), dtype=stack.dtype)))
    return torch.stack(maps)


# ---- image contents for the device tests (float32, (B,3,H,W)) ------------------------------------------------------------
def noise_image(B, H, W, seed):
    """iid uniform [0, 1): colour distances of about 0.5, affinities down to underflow at small sigma_color."""
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


def flat_image(B, H, W, value=0.375):
    return torch.full((B, 3, H, W), value)


def step_image(B, H, W):
    """A vertical step edge: 0 left of W // 2, 1 from there on."""
    img = torch.zeros(B, 3, H, W)
    img[..., W // 2:] = 1.0
    return img
