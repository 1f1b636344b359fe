"""Oracle of the device-wide component labelling, seeded region growing and its balanced weights (csrc/components_grid.hip):
numpy + scipy.ndimage, no device code.  ``components`` is ``ndimage.label`` per value, relabelled to the raster index of each
component's first pixel; ``grow`` is the DSRG rule built on it (``grow_by_propagation`` states the same rule another way, per
class with ``ndimage.binary_propagation``: tests/test_srg.py holds the two against each other); ``weights`` are the formulas of
``ops.balanced_seed_weights`` in float64.  The case list and the input recipes of tests/test_hip_srg.py live here too."""
import functools

import numpy as np
from scipy import ndimage

IGNORE = 255
EIGHT = np.ones((3, 3), dtype=bool)
FOUR = ndimage.generate_binary_structure(2, 1)

# (B, C, H, W): components across every kind of tile seam (the tiles are 64 wide, 32 high) and off every multiple; 1x2x33x65
# is one pixel over a tile in each direction, 1x2x256x257 is past the 65 535 pixels the one-workgroup kernel keeps in LDS
SHAPES = [(1, 2, 1, 1), (1, 2, 1, 7), (1, 2, 7, 1), (2, 3, 5, 7), (3, 3, 37, 53), (2, 21, 64, 64), (2, 2, 65, 130), (1, 3, 3, 300),
          (1, 2, 300, 3), (2, 2, 96, 130), (1, 2, 33, 65), (1, 2, 256, 257)]


def structure(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity!r}: 4 or 8")
    return EIGHT if connectivity == 8 else FOUR


def components(labels, background=None, connectivity=8, want_area=False):
    """int32 (B,H,W): the raster index y W + x of the first pixel of every pixel's component (same value, connected), -1
    where ``labels == background``; with ``want_area`` also the component's pixel count per pixel (0 on background)."""
    labels = np.asarray(labels)
    st = structure(connectivity)
    B, H, W = labels.shape
    comp = np.full((B, H * W), -1, dtype=np.int32)
    area = np.zeros((B, H * W), dtype=np.int32)
    idx = np.arange(H * W)
    for b in range(B):
        for v in np.unique(labels[b]):
            if background is not None and v == background:
                continue
            lab, n = ndimage.label(labels[b] == v, structure=st)
            flat = lab.ravel()
            first = np.full(n + 1, H * W, dtype=np.int64)
            np.minimum.at(first, flat, idx)
            m = flat > 0
            comp[b, m] = first[flat[m]]
            area[b, m] = np.bincount(flat, minlength=n + 1)[flat[m]]
    comp, area = comp.reshape(B, H, W), area.reshape(B, H, W)
    return (comp, area) if want_area else comp


def candidates(scores, thresh, present=None):
    """int64 (B,H,W): the class a pixel is a candidate of (the first index of the largest score over the present classes, if
    that score is > its threshold in float32; a NaN among the present scores: none), -1 for none."""
    s = np.asarray(scores, dtype=np.float32)
    B, C, H, W = s.shape
    thresh = np.asarray(thresh, dtype=np.float32).reshape(C)
    pres = np.ones((B, C), dtype=bool) if present is None else np.asarray(present).astype(bool)
    pres4 = np.broadcast_to(pres[:, :, None, None], s.shape)
    nan = (np.isnan(s) & pres4).any(axis=1)
    masked = np.where(pres4 & ~np.isnan(s), s, -np.inf)
    a = np.argmax(masked, axis=1)                                            # the first index of the maximum
    top = np.take_along_axis(s, a[:, None], axis=1)[:, 0]
    a_present = np.take_along_axis(pres4, a[:, None], axis=1)[:, 0]
    with np.errstate(invalid="ignore"):
        ok = ~nan & a_present & (top > thresh[a])
    return np.where(ok, a, -1).astype(np.int64)


def _finish(seeds, cand, grows, C, ignore_index):
    seeds = np.asarray(seeds).astype(np.int64)
    seeded = (seeds >= 0) & (seeds < C)
    grown = np.where(seeded, seeds, np.where(grows, cand, ignore_index)).astype(np.int64)
    B = grown.shape[0]
    counts = np.stack([np.bincount(grown[b][(grown[b] >= 0) & (grown[b] < C)].ravel(), minlength=C) for b in range(B)]).astype(np.int64)
    return grown, counts


def grow(scores, seeds, thresh, present=None, ignore_index=IGNORE, stats=None):
    """(grown, counts) of ``ops.seeded_region_growing``.  ``stats`` (a dict) receives the number of candidate components and of
    those that grow."""
    C = np.asarray(scores).shape[1]
    cand = candidates(scores, thresh, present)
    comp = components(cand, background=-1, connectivity=8)
    seeds = np.asarray(seeds).astype(np.int64)
    hit = (cand >= 0) & (seeds == cand)
    grows = np.zeros(cand.shape, dtype=bool)
    n_comp = n_grown = 0
    for b in range(cand.shape[0]):
        roots = np.unique(comp[b][hit[b]])
        grows[b] = (cand[b] >= 0) & np.isin(comp[b], roots)
        n_comp += len(np.unique(comp[b][cand[b] >= 0]))
        n_grown += len(roots)
    if stats is not None:
        stats.update(components=n_comp, grown=n_grown)
    return _finish(seeds, cand, grows, C, ignore_index)


def grow_by_propagation(scores, seeds, thresh, present=None, ignore_index=IGNORE):
    """The same rule without component labels: per class, the candidates reachable from a seed of that class."""
    C = np.asarray(scores).shape[1]
    cand = candidates(scores, thresh, present)
    seeds = np.asarray(seeds).astype(np.int64)
    grows = np.zeros(cand.shape, dtype=bool)
    for b in range(cand.shape[0]):
        for c in range(C):
            m = cand[b] == c
            if m.any():
                grows[b] |= ndimage.binary_propagation((seeds[b] == c) & m, mask=m, structure=EIGHT)
    return _finish(seeds, cand, grows, C, ignore_index)


def weights(grown, counts, balance="fg_bg"):
    """float64 (B,H,W): 1 / (B n) with n the pixel count of the pixel's group in its image ('fg_bg': class 0 / classes >= 1,
    'class': every class), 'none': 1; 0 at a label outside [0,C) and for a group without a pixel."""
    grown, counts = np.asarray(grown), np.asarray(counts).astype(np.float64)
    B, C = counts.shape
    lab = (grown >= 0) & (grown < C)
    g = np.where(lab, grown, 0)
    if balance == "none":
        return lab.astype(np.float64)
    if balance == "fg_bg":
        n = np.stack([counts[:, 0], counts[:, 1:].sum(axis=1)], axis=1)
        g = np.minimum(g, 1)
    elif balance == "class":
        n = counts
    else:
        raise ValueError(f"balance {balance!r}")
    npix = np.take_along_axis(n, g.reshape(B, -1), axis=1).reshape(g.shape)
    with np.errstate(divide="ignore"):
        w = np.where(npix > 0, 1.0 / (B * npix), 0.0)
    return np.where(lab, w, 0.0)


def seeding_loss(logits, grown, pixel_weight, balance, dtype):
    """The criterion's loss and gradient in torch ``dtype`` on the CPU from given grown labels and pixel weights (the weights ARE
    float32 values by definition: ``float(1.0 / double(B n))``): sum_p w_p (-log softmax(logits)_grown(p)), divided by sum w
    for balance 'none'."""
    import torch
    z = torch.as_tensor(np.asarray(logits)).to(dtype).requires_grad_()
    g = torch.as_tensor(np.asarray(grown)).long()
    w = torch.as_tensor(np.asarray(pixel_weight)).to(dtype)
    C = z.shape[1]
    lab = (g >= 0) & (g < C)
    nll = -torch.log_softmax(z, dim=1).gather(1, torch.where(lab, g, torch.zeros_like(g))[:, None])[:, 0]
    loss = (torch.where(lab, w, torch.zeros_like(w)) * nll).sum()
    if balance == "none":
        loss = loss / torch.where(lab, w, torch.zeros_like(w)).sum()
    loss.backward()
    return loss.detach(), z.grad


# ------------------------------------------------------------------------------------------------ recipes
def thresholds(C):
    return np.array([0.7] + [0.55] * (C - 1), dtype=np.float32)


def make_scores(B, C, H, W, seed):
    """float32 (B,C,H,W): the softmax of three random low-frequency sinusoids per class (amplitude about 2) plus 0.05 noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    z = np.zeros((B, C, H, W))
    for b in range(B):
        for c in range(C):
            for _ in range(3):
                fy, fx = rng.uniform(-3, 3, 2)
                z[b, c] += 2.0 / 1.5 * np.sin(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
    z += 0.05 * rng.standard_normal(z.shape)
    z -= z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def make_seeds(scores, seed, ignore=IGNORE):
    """int64 (B,H,W): seeds on 2 % of the pixels (30 % of a map below 100 pixels) with the argmax class, 10 % of them
    replaced by a random class; ``ignore`` elsewhere."""
    rng = np.random.default_rng(seed)
    B, C, H, W = scores.shape
    frac = 0.3 if H * W < 100 else 0.02
    a = scores.argmax(axis=1)
    cls = np.where(rng.random((B, H, W)) < 0.1, rng.integers(0, C, (B, H, W)), a)
    return np.where(rng.random((B, H, W)) < frac, cls, ignore).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(i):
    """(scores, seeds, thresh, grown, counts, stats) of SHAPES[i] - made once, shared, never written.  From 5 x 7 upwards at
    least one component grows and at least one does not: a degenerate recipe would hide a failure."""
    B, C, H, W = SHAPES[i]
    scores = make_scores(B, C, H, W, 100 + i)
    seeds = make_seeds(scores, 200 + i)
    thresh = thresholds(C)
    stats = {}
    grown, counts = grow(scores, seeds, thresh, stats=stats)
    if H * W >= 35:
        assert 0 < stats["grown"] < stats["components"], (SHAPES[i], stats)
    for a in (scores, seeds, thresh, grown, counts):
        a.setflags(write=False)
    return scores, seeds, thresh, grown, counts, stats


# ------------------------------------------------------------------------------------------------ structured label maps
def spiral(H, W):
    """A one-pixel-wide spiral of 1s on 0s, wound inwards with a one-pixel gap."""
    m = np.zeros((H, W), dtype=np.int64)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] == 0

    while True:
        for _ in range(2):                               # straight on, else one turn to the right
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = 1


def serpentine(H, W):
    """A one-pixel-wide path that fills every other row and turns at alternating ends: one component, the longest chain."""
    m = np.zeros((H, W), dtype=np.int64)
    m[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def checkerboard(H, W):
    yy, xx = np.indices((H, W))
    return ((yy + xx) % 2).astype(np.int64)


def comb(H, W, vertical):
    m = np.zeros((H, W), dtype=np.int64)
    if vertical:
        m[:, 0::2] = 1
        m[H - 1, :] = 1
    else:
        m[0::2, :] = 1
        m[:, W - 1] = 1
    return m


def structured_maps():
    """name -> (B,H,W) int64 label maps at 65 x 130 (tile seams in both directions, one pixel over two tile rows)."""
    H, W = 65, 130
    rng = np.random.default_rng(7)
    one = lambda m: m[None]                                                    # noqa: E731
    maps = {
        "spiral": one(spiral(H, W)),
        "serpentine": one(serpentine(H, W)),
        "checkerboard": one(checkerboard(H, W)),
        "full": np.ones((1, H, W), dtype=np.int64),
        "comb_vertical": one(comb(H, W, True)),
        "comb_horizontal": one(comb(H, W, False)),
        "all_background": np.zeros((1, H, W), dtype=np.int64),
        "three_different": np.stack([spiral(H, W), checkerboard(H, W), (rng.random((H, W)) < 0.55).astype(np.int64)]),
        "three_identical": np.stack([serpentine(H, W)] * 3),
        "random_1": np.full((2, H, W), 3, dtype=np.int64),
        "random_2": (rng.random((2, H, W)) < 0.6).astype(np.int64),
        "random_21": rng.integers(0, 21, (2, H, W)).astype(np.int64),
        "random_2_past_lds": (rng.random((1, 256, 257)) < 0.6).astype(np.int64),
    }
    return maps
