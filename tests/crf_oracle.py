"""CPU oracle of dense-CRF refinement (reference AlternatingDirectionCutLoss.py:183-204, pydensecrf defaults), written from
the published algorithm: the permutohedral lattice of Adams et al. 2010 as densecrf builds it, mean-field inference with
symmetric normalisation and Potts compatibilities.  Vectorised numpy.

  * lattice build (features, elevation, remainder-0 point, rank, barycentric weights, vertex keys) in float32, operation
    by operation as the device does it - the keys and weights must come out bit-identical;
  * unique lattice points by np.unique on an exact integer code of the key, blur neighbours by np.searchsorted;
  * splat / blur / slice and the mean field in float64;
  * an exact dense filter exp(-|f_i - f_j|^2 / 2) by brute force in float64 (small images only).

Not verified against pydensecrf itself (no machine here has it): DESIGN.md section 7.
"""
import math

import numpy as np


def lattice_scale(d):
    """densecrf: inv_std_dev = sqrt(2/3) (d+1) as float, scale[i] = 1/sqrt((i+1)(i+2)) * inv_std_dev in double -> float."""
    inv = float(np.float32(math.sqrt(2.0 / 3.0) * (d + 1)))
    return np.array([1.0 / math.sqrt((i + 2) * (i + 1)) * inv for i in range(d)], dtype=np.float32)


def crf_features(rgb, sxy, srgb=None):
    """(H,W,3) uint8 -> (N, d) float32 features in raster order j*W+i: (i/sxy, j/sxy[, r/srgb, g/srgb, b/srgb])."""
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    f = [xx.ravel().astype(np.float32) / np.float32(sxy), yy.ravel().astype(np.float32) / np.float32(sxy)]
    if srgb is not None:
        f += [rgb[..., c].ravel().astype(np.float32) / np.float32(srgb) for c in range(3)]
    return np.stack(f, 1)


def lattice_coords(f):
    """(N, d) float32 features -> keys (N, d+1, d) int64 and barycentric weights (N, d+1) float32."""
    f = np.asarray(f, dtype=np.float32)
    N, d = f.shape
    D = d + 1
    sc = lattice_scale(d)
    elev = np.zeros((N, D), np.float32)
    sm = np.zeros(N, np.float32)
    for j in range(d, 0, -1):
        cf = f[:, j - 1] * sc[j - 1]
        elev[:, j] = sm - np.float32(j) * cf
        sm = sm + cf
    elev[:, 0] = sm
    down = np.float32(1.0) / np.float32(D)          # the reciprocal in float, as densecrf's down_factor
    v = elev * down
    up = np.ceil(v) * np.float32(D)
    dn = np.floor(v) * np.float32(D)
    rem0 = np.where(up - elev < elev - dn, up, dn).astype(np.int64)
    s = rem0.sum(1) // D                            # every rem0 is a multiple of d+1: exact
    rank = np.zeros((N, D), np.int64)
    for i in range(d):
        di = elev[:, i] - rem0[:, i].astype(np.float32)
        for j in range(i + 1, D):
            lt = di < elev[:, j] - rem0[:, j].astype(np.float32)
            rank[:, i] += lt
            rank[:, j] += ~lt
    rank += s[:, None]
    lo, hi = rank < 0, rank > d
    rank[lo] += D
    rem0[lo] += D
    rank[hi] -= D
    rem0[hi] -= D
    bc = np.zeros((N, D + 1), np.float32)
    rows = np.arange(N)
    for i in range(D):
        v = (elev[:, i] - rem0[:, i].astype(np.float32)) * down
        bc[rows, d - rank[:, i]] += v
        bc[rows, d - rank[:, i] + 1] -= v
    bc[:, 0] += np.float32(1.0) + bc[:, D]
    keys = np.empty((N, D, d), np.int64)
    for r in range(D):
        keys[:, r, :] = rem0[:, :d] + np.where(rank[:, :d] <= d - r, r, r - D)
    return keys, bc[:, :D]


class Lattice:
    """The permutohedral lattice of one image's features."""

    def __init__(self, f):
        self.keys, self.bary = lattice_coords(f)
        N, D, d = self.keys.shape
        self.N, self.d = N, d
        flat = self.keys.reshape(-1, d)
        lo = flat.min(0) - (d + 2)
        span = flat.max(0) - lo + d + 3
        mult = np.ones(d, np.int64)
        for i in range(d - 2, -1, -1):
            mult[i] = mult[i + 1] * span[i + 1]
        assert int(np.prod([int(x) for x in span])) < (1 << 62), "key code overflow"
        code = ((flat - lo) * mult).sum(1)
        uniq, inv = np.unique(code, return_inverse=True)
        self.M = len(uniq)
        self.off = inv.reshape(N, D)
        self.nbr = []
        for j in range(D):
            pair = []
            for sgn in (-1, 1):              # n1 = key - 1 (key[j] + d at axis j), n2 = key + 1 (key[j] - d)
                delta = np.full(d, sgn, np.int64)
                if j < d:
                    delta[j] = -sgn * d
                c = uniq + int((delta * mult).sum())
                pos = np.searchsorted(uniq, c)
                found = (pos < self.M) & (uniq[np.minimum(pos, self.M - 1)] == c)
                pair.append(np.where(found, pos, self.M))      # row M holds zeros: a missing neighbour
            self.nbr.append(pair)
        self.alpha = 1.0 / (1.0 + 2.0 ** (-d))

    def apply(self, vals, reverse=False):
        """Lattice(vals): (N, L) -> (N, L), float64.  reverse: the blur axes in the opposite order - the transpose of the
        forward filter (on a sparse lattice the per-axis blurs do not commute, so the filter itself is not symmetric)."""
        vals = np.asarray(vals, np.float64).reshape(self.N, -1)
        w = self.bary.astype(np.float64)
        V = np.zeros((self.M + 1, vals.shape[1]))
        for l in range(vals.shape[1]):
            V[:self.M, l] = np.bincount(self.off.ravel(), weights=(w * vals[:, None, l]).ravel(), minlength=self.M)
        for n1, n2 in (self.nbr[::-1] if reverse else self.nbr):
            Vn = V.copy()
            Vn[:self.M] = V[:self.M] + 0.5 * (V[n1] + V[n2])
            V = Vn
        return self.alpha * (w[:, :, None] * V[self.off]).sum(1)


class NormalisedFilter:
    """K~ x = n * K(n * x), n = 1/sqrt(K 1 + 1e-20) (NORMALIZE_SYMMETRIC).  K: a Lattice, or exact=True the dense
    Gaussian exp(-|f_i - f_j|^2 / 2) in float64."""

    def __init__(self, f, exact=False):
        if exact:
            g = np.asarray(f, np.float64)
            sq = ((g[:, None, :] - g[None, :, :]) ** 2).sum(-1)
            Kd = np.exp(-0.5 * sq)
            self.K = lambda x: Kd @ x
        else:
            lat = Lattice(f)
            self.K = lat.apply
        N = len(f)
        self.n = 1.0 / np.sqrt(self.K(np.ones((N, 1)))[:, 0] + 1e-20)

    def __call__(self, x):
        x = np.asarray(x, np.float64).reshape(len(self.n), -1)
        return self.n[:, None] * self.K(self.n[:, None] * x)


def unary_from_cam(cam, cam_thresh=None):
    """(H,W) CAM -> (2, N) float32: threshold (values kept), clip [1e-8, 1], unary_from_softmax's clip [1e-5, 1], -log."""
    cam = np.array(cam, dtype=np.float32)
    if cam_thresh is not None:
        cam[cam < np.float32(cam_thresh)] = 0
    probs = np.clip(np.stack([np.float32(1) - cam, cam]), np.float32(1e-8), np.float32(1))
    return -np.log(np.clip(probs, np.float32(1e-5), np.float32(1))).reshape(2, -1).astype(np.float32)


def _softmax(t):
    t = t - t.max(0, keepdims=True)
    e = np.exp(t)
    return e / e.sum(0, keepdims=True)


def dense_crf(rgb, cam=None, cam_thresh=None, n_iter=5, gauss=(1, 2), bilateral=(50, 5, 10), exact=False, unary=None):
    """One image: rgb (H,W,3) uint8, cam (H,W) (or unary (2,H,W)) -> mask (H,W) uint8, Q (2,H,W) float64."""
    H, W = rgb.shape[:2]
    U = (unary_from_cam(cam, cam_thresh) if unary is None else np.asarray(unary, np.float32).reshape(2, -1)).astype(np.float64)
    terms = [(NormalisedFilter(crf_features(rgb, gauss[0]), exact), gauss[1]),
             (NormalisedFilter(crf_features(rgb, bilateral[0], bilateral[1]), exact), bilateral[2])]
    Q = _softmax(-U)
    for _ in range(n_iter):
        tmp = -U
        for filt, w in terms:
            tmp = tmp + w * filt(Q.T).T
        Q = _softmax(tmp)
    mask = (Q[1] > Q[0]).astype(np.uint8)           # argmax, ties -> label 0
    return mask.reshape(H, W), Q.reshape(2, H, W)


def quantise(img):
    """(3,H,W) float in [0,1] -> (H,W,3) uint8: the notebook's (img*255).astype(np.uint8) (truncation)."""
    x = np.asarray(img, np.float32).transpose(1, 2, 0) * np.float32(255)
    return np.clip(x, 0, 255).astype(np.uint8)
