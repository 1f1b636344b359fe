"""Oracle of the integer SLIC superpixels and of the pooling over them (csrc/slic.hip): vectorised numpy + scipy.ndimage, no
device code.  It restates the contract of include/wsdl_hip.h "SLIC superpixels, superpixel pooling": all arithmetic is integer
(int64 here), ``//`` floors non-negative numbers.  ``slic`` returns every stage (raw, centres, segments, n_segments);
``components4`` is ``ndimage.label`` with the 4-connected structure per label value, relabelled to first-pixel indices;
``superpixel_mean`` / ``superpixel_snap`` / ``superpixel_vote`` are the pooling rules.  The geometry list, the image recipes and
the parameter grid of tests/test_hip_slic.py live here too; tests/test_slic.py holds this file against independent loops."""
import functools

import numpy as np
from scipy import ndimage

FOUR = ndimage.generate_binary_structure(2, 1)
IGNORE = 255

# (B, H, W, step): the smallest sizes at which each stage can go wrong - one pixel, one row / column, cells that tile exactly
# (64 / 16), seams of the labelling's 64 x 32 tiles (65 x 130), one cell (step 64 on 20 x 30), more than one block of the rank
# scan (2048 pixels) and of its block counts; the last one has step 1: one centre per pixel, the window of an assignment tile no
# longer fits on chip and the kernel takes its global-memory path
SHAPES = [(1, 1, 1, 4), (1, 1, 7, 2), (1, 7, 1, 2), (2, 5, 7, 3), (1, 37, 53, 8), (2, 64, 64, 16), (2, 65, 130, 10), (1, 3, 300, 4),
          (1, 300, 3, 4), (1, 20, 30, 64), (1, 96, 130, 16), (1, 256, 257, 16), (1, 40, 70, 1)]
COMPACTNESS = (1, 10, 40)
NUM_ITER = (0, 1, 10)


def default_min_size(step):
    return max(1, step * step // 4)


def max_segments(H, W, step, min_size=None):
    GH, GW = grid(H, W, step)
    return GH * GW + (H * W) // (default_min_size(step) if min_size is None else min_size) + 1


def grid(H, W, S):
    return max(1, (H + S // 2) // S), max(1, (W + S // 2) // S)


def initial_centres(img, S):
    """(K,5) int64 for one image (3,H,W) uint8."""
    _, H, W = img.shape
    GH, GW = grid(H, W, S)
    cy = ((2 * np.arange(GH) + 1) * H) // (2 * GH)
    cx = ((2 * np.arange(GW) + 1) * W) // (2 * GW)
    yy, xx = np.meshgrid(cy, cx, indexing="ij")
    col = img[:, yy, xx].astype(np.int64)                                   # (3,GH,GW)
    return np.stack([16 * yy, 16 * xx, 16 * col[0], 16 * col[1], 16 * col[2]], axis=-1).reshape(GH * GW, 5).astype(np.int64)


def assign(img, centres, S, m):
    """(H,W) int64 labels of one image against (K,5) centres."""
    _, H, W = img.shape
    GH, GW = grid(H, W, S)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    hy, hx = np.minimum(GH - 1, y * GH // H), np.minimum(GW - 1, x * GW // W)
    I = img.astype(np.int64) * 16
    best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    lab = np.zeros((H, W), dtype=np.int64)
    for dy in (-1, 0, 1):                                                   # ascending k: a strict < keeps the smallest on ties
        for dx in (-1, 0, 1):
            cy, cx = hy + dy, hx + dx
            ok = (cy >= 0) & (cy < GH) & (cx >= 0) & (cx < GW)
            k = np.where(ok, cy * GW + cx, 0)
            c = centres[k]                                                  # (H,W,5)
            D = S * S * ((I[0] - c[..., 2]) ** 2 + (I[1] - c[..., 3]) ** 2 + (I[2] - c[..., 4]) ** 2) \
                + m * m * ((16 * y - c[..., 0]) ** 2 + (16 * x - c[..., 1]) ** 2)
            take = ok & (D < best)
            best = np.where(take, D, best)
            lab = np.where(take, k, lab)
    return lab


def update(img, lab, centres):
    _, H, W = img.shape
    K = centres.shape[0]
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    flat = lab.ravel()
    n = np.bincount(flat, minlength=K).astype(np.int64)
    out = centres.copy()
    has = n > 0
    for j, q in enumerate((y, x, img[0], img[1], img[2])):
        s = np.zeros(K, dtype=np.int64)
        np.add.at(s, flat, q.ravel().astype(np.int64))
        out[has, j] = (16 * s[has] + n[has] // 2) // n[has]
    return out


def components4(lab):
    """(comp, area) of one (H,W) label map, 4-connected, every value: the raster index of the component's first pixel and the
    component's pixel count, at every pixel."""
    H, W = lab.shape
    comp = np.full(H * W, -1, dtype=np.int64)
    area = np.zeros(H * W, dtype=np.int64)
    idx = np.arange(H * W).reshape(H, W)
    shifted = lab.astype(np.int64) - lab.min() + 1
    for v, sl in enumerate(ndimage.find_objects(shifted), start=1):
        if sl is None:
            continue
        cl, n = ndimage.label(shifted[sl] == v, structure=FOUR)
        flat, pos = cl.ravel(), idx[sl].ravel()
        first = np.full(n + 1, H * W, dtype=np.int64)
        np.minimum.at(first, flat, pos)
        mk = flat > 0
        comp[pos[mk]] = first[flat[mk]]
        area[pos[mk]] = np.bincount(flat, minlength=n + 1)[flat[mk]]
    return comp.reshape(H, W), area.reshape(H, W)


def enforce_connectivity(raw, min_size, stats=None):
    """(segments int32 (H,W), n) of one raw label map: the orphan rule of the contract, chains resolved by pointer jumping."""
    H, W = raw.shape
    comp, area = components4(raw)
    roots = np.flatnonzero(comp.ravel() == np.arange(H * W))               # first pixels, ascending
    r_area, r_lab = area.ravel()[roots], raw.ravel()[roots]
    order = np.lexsort((roots, -r_area, r_lab))                             # per label: largest area, then smallest first pixel
    main = np.zeros(len(roots), dtype=bool)
    main[order[np.r_[True, r_lab[order][1:] != r_lab[order][:-1]]]] = True
    orphan = ~main & (r_area < min_size) & (roots != 0)
    nb = np.where(roots % W > 0, roots - 1, roots - W)
    parent = np.where(orphan, comp.ravel()[np.where(orphan, nb, 0)], roots)  # as first-pixel indices
    pos = np.full(H * W, -1, dtype=np.int64)
    pos[roots] = np.arange(len(roots))
    par = pos[parent]
    assert (par[orphan] < np.flatnonzero(orphan)).all()                     # the neighbour's component starts earlier
    depth = 0
    while True:
        nxt = par[par]
        if np.array_equal(nxt, par):
            break
        par = nxt
        depth += 1
    kept = ~orphan
    rank = np.cumsum(kept) - 1
    seg = rank[par][pos[comp.ravel()]].reshape(H, W).astype(np.int32)
    if stats is not None:
        stats["components"] = stats.get("components", 0) + len(roots)
        stats["orphans"] = stats.get("orphans", 0) + int(orphan.sum())
        stats["chain"] = max(stats.get("chain", 0), chain_length(pos[parent], orphan))
    return seg, int(kept.sum())


def chain_length(par, orphan):
    """The longest chain of orphans (in components) that ends at a kept component."""
    length = np.zeros(len(par), dtype=np.int64)
    for i in np.flatnonzero(orphan):                                        # ascending: the parent's length is final
        length[i] = length[par[i]] + 1
    return int(length.max()) if len(par) else 0


def slic(images, step, compactness=10, num_iter=10, min_size=None, stats=None):
    """dict(raw int32 (B,H,W), centres int32 (B,K,5), segments int32 (B,H,W), n_segments int32 (B,)) for uint8 (B,3,H,W)."""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim == 4 and images.shape[1] == 3
    B, _, H, W = images.shape
    min_size = default_min_size(step) if min_size is None else min_size
    raws, cens, segs, ns = [], [], [], []
    for b in range(B):
        c = initial_centres(images[b], step)
        lab = None
        for _ in range(num_iter):
            lab = assign(images[b], c, step, compactness)
            c = update(images[b], lab, c)
        if lab is None:
            lab = assign(images[b], c, step, compactness)
        seg, n = enforce_connectivity(lab, min_size, stats)
        raws.append(lab)
        cens.append(c)
        segs.append(seg)
        ns.append(n)
    return {"raw": np.stack(raws).astype(np.int32), "centres": np.stack(cens).astype(np.int32), "segments": np.stack(segs),
            "n_segments": np.array(ns, dtype=np.int32)}


# ------------------------------------------------------------------------------------------------ pooling
def quantise(values):
    """int64 q = rint(double(clamp(v, -2^15, 2^15)) 2^24) (ties to even, as llrint), 0 at a NaN."""
    v = np.asarray(values, dtype=np.float32)
    nan = np.isnan(v)
    c = np.clip(np.where(nan, np.float32(0), v), np.float32(-32768), np.float32(32768)).astype(np.float64)
    return np.rint(c * 16777216.0).astype(np.int64), nan


def superpixel_mean(values, segments, n_max):
    """(mean float32 (B,C,n_max), count int32 (B,n_max)); pixels whose id is outside [0, n_max) are not pooled."""
    values, segments = np.asarray(values, dtype=np.float32), np.asarray(segments)
    B, C, H, W = values.shape
    q, nan = quantise(values)
    mean = np.zeros((B, C, n_max), dtype=np.float32)
    count = np.zeros((B, n_max), dtype=np.int32)
    for b in range(B):
        s = segments[b].ravel().astype(np.int64)
        ok = (s >= 0) & (s < n_max)
        n = np.bincount(s[ok], minlength=n_max)
        count[b] = n
        for c in range(C):
            tot = np.zeros(n_max, dtype=np.int64)
            np.add.at(tot, s[ok], q[b, c].ravel()[ok])
            bad = np.zeros(n_max, dtype=bool)
            bad[s[ok & nan[b, c].ravel()]] = True
            with np.errstate(divide="ignore", invalid="ignore"):
                m = (tot.astype(np.float64) / (n.astype(np.float64) * 16777216.0)).astype(np.float32)
            m[n == 0] = 0
            m[bad] = np.nan
            mean[b, c] = m
    return mean, count


def superpixel_snap(values, segments, n_max):
    mean, _ = superpixel_mean(values, segments, n_max)
    segments = np.asarray(segments)
    ok = (segments >= 0) & (segments < n_max)
    s = np.where(ok, segments, 0)
    out = np.take_along_axis(mean, s.reshape(s.shape[0], 1, -1).astype(np.int64), axis=2).reshape(np.asarray(values).shape)
    return np.where(ok[:, None], out, np.float32(0)).astype(np.float32)


def superpixel_vote(labels, segments, n_max, num_classes, ignore_index=IGNORE):
    labels, segments = np.asarray(labels).astype(np.int64), np.asarray(segments).astype(np.int64)
    out = np.full(labels.shape, ignore_index, dtype=np.int64)
    for b in range(labels.shape[0]):
        ok = (segments[b] >= 0) & (segments[b] < n_max) & (labels[b] >= 0) & (labels[b] < num_classes)
        cnt = np.zeros((n_max, num_classes), dtype=np.int64)
        np.add.at(cnt, (segments[b][ok], labels[b][ok]), 1)
        win = np.where(cnt.max(axis=1) > 0, cnt.argmax(axis=1), -1)         # argmax: the first (smallest) class on ties
        inside = (segments[b] >= 0) & (segments[b] < n_max)
        w = win[np.where(inside, segments[b], 0)]
        out[b] = np.where(inside & (w >= 0), w, ignore_index)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def make_image(kind, H, W, seed=0):
    """One uint8 (3,H,W) image."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "flat":
        img = np.broadcast_to(np.array([90, 140, 200]).reshape(3, 1, 1), (3, H, W))
    elif kind == "halves":                                                  # the edge sits off every grid of the steps used
        edge = (x > (5 * W) // 11) if W > 1 else (y > (5 * H) // 11)
        img = np.where(edge[None], np.array([220, 40, 90]).reshape(3, 1, 1), np.array([30, 180, 60]).reshape(3, 1, 1))
    elif kind == "checker":
        img = np.where(((y + x) % 2 == 0)[None], 255, 0) * np.ones((3, 1, 1), dtype=np.int64)
    elif kind == "noise":
        img = rng.integers(0, 256, (3, H, W))
    elif kind == "blobs":
        img = np.zeros((3, H, W))
        for _ in range(6):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.1, 0.35) * max(H, W, 4)
            col = rng.uniform(-120, 120, (3, 1, 1))
            img = img + col * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))[None]
        img = np.clip(np.rint(img + 128), 0, 255)
    elif kind == "ramp":
        img = np.broadcast_to(((x * 255) // max(1, W - 1))[None], (3, H, W))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(img).astype(np.uint8)


CONTENTS = ("flat", "halves", "checker", "noise", "blobs", "ramp", "same3", "different3")


def make_batch(content, B, H, W, seed=0):
    """uint8 (B,3,H,W); ``same3`` / ``different3`` are batches of three images whatever ``B``."""
    if content == "same3":
        return np.stack([make_image("blobs", H, W, seed)] * 3)
    if content == "different3":
        return np.stack([make_image(k, H, W, seed + i) for i, k in enumerate(("blobs", "noise", "halves"))])
    return np.stack([make_image(content, H, W, seed + b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def structured_images():
    """name -> uint8 (B,3,H,W): every content at 2x65x130 (which crosses the labelling's tile seams)."""
    out = {}
    for c in CONTENTS:
        a = make_batch(c, 2, 65, 130, seed=11)
        a.setflags(write=False)
        out[c] = a
    return out


@functools.lru_cache(maxsize=None)
def case(content, shape, compactness=10, num_iter=10, min_size=None):
    """(images, expected dict, stats) - computed once and shared by the tests; the arrays are read-only."""
    B, H, W, step = shape
    images = structured_images()[content] if (H, W) == (65, 130) and B == 2 else make_batch(content, B, H, W, seed=7)
    stats = {}
    want = slic(images, step, compactness, num_iter, min_size, stats=stats)
    images = np.array(images)
    for a in [images] + list(want.values()):
        a.setflags(write=False)
    return images, want, stats


def device_cases():
    """The pruned grid of tests/test_hip_slic.py: every geometry on blobs and on noise with the defaults, every content at 2x65x130
    with the defaults, and the parameter grid (compactness x num_iter x min_size) on noise at 1x37x53x8 and 2x65x130x10."""
    cases = []
    for s in SHAPES:
        cases.append(("blobs", s, 10, 10, None))
        cases.append(("noise", s, 10, 10, None))
    for c in CONTENTS:
        cases.append((c, (2, 65, 130, 10), 10, 10, None))
    for s in ((1, 37, 53, 8), (2, 65, 130, 10)):
        for m in COMPACTNESS:
            for it in NUM_ITER:
                for ms in (1, None, s[1] * s[2] + 1):
                    cases.append(("noise", s, m, it, ms))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out
