"""numpy restatement of Pillow's 8-bit resampling (``Image.resize(size, BILINEAR | BICUBIC)`` on modes "RGB" / "L",
``box=None``, ``reducing_gap=None``) - the oracle of csrc/pil_resize.hip, beside crf_oracle.py.

Per axis: ``scale = in / out``, ``fscale = max(scale, 1)``, ``support = s * fscale`` (s = 1 BILINEAR, 2 BICUBIC),
``ksize = int(ceil(support)) * 2 + 1``; for output index xx: ``center = (xx + 0.5) * scale``,
``xmin = max(int(center - support + 0.5), 0)``, ``xmax = min(int(center + support + 0.5), in) - xmin``, weights
``f((x + xmin - center + 0.5) * (1 / fscale))`` summed left to right and divided by the sum when it is non-zero - all in
float64, which is C double (numpy's element-wise operations and ``cumsum`` do not reassociate or contract).  Coefficients get
22 fractional bits, rounded half away from zero.  A pass is ``clamp((2^21 + sum pixel * k) >> 22, 0, 255)``; the horizontal
pass runs first and its uint8 result feeds the vertical pass; a pass whose in == out is skipped.
"""
import numpy as np

BILINEAR, BICUBIC = 2, 3          # Pillow's Image.BILINEAR / Image.BICUBIC
PRECISION_BITS = 22

# the sizes the device kernel is pinned on (H, W): down- and up-sampling, identity, odd sides, a side of 1
SIZES = [(375, 500), (500, 333), (224, 224), (224, 500), (137, 91), (1024, 768), (300, 224), (64, 3000), (225, 223), (2, 2),
         (1, 37)]
TARGETS = [(BICUBIC, (224, 224)), (BILINEAR, (256, 256))]


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def coeffs(n_in, n_out, filt):
    """(ksize, bounds (n_out, 2) int32 = (xmin, xmax), kk (n_out, ksize) int32)."""
    f, s = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}[filt]
    scale = np.float64(n_in) / np.float64(n_out)
    fscale = max(scale, np.float64(1.0))
    support = s * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    inside = x < xmax[:, None]
    w = f(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(inside, w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                     # left to right; the zeros beyond xmax change nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    w = np.where(inside, w, 0.0)
    scaled = w * np.float64(1 << PRECISION_BITS)
    kk = np.where(w < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)
    return ksize, np.stack([xmin, xmax], axis=1).astype(np.int32), kk


def _pass_axis1(img, n_out, filt):
    """Resample axis 1 of (A, n_in, C) uint8."""
    n_in = img.shape[1]
    if n_in == n_out:
        return img
    _, bounds, kk = coeffs(n_in, n_out, filt)
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], n_out, img.shape[2]), dtype=np.uint8)
    for xx in range(n_out):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + xmax], kk[xx, :xmax].astype(np.int64),
                                                         axes=([1], [0]))
        assert np.abs(acc).max(initial=0) < 2 ** 31       # Pillow sums in int32
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, size, filt):
    """img (H, W) or (H, W, C) uint8 -> size = (out_h, out_w), as ``Image.fromarray(img).resize((out_w, out_h), filt)``."""
    a = np.asarray(img)
    assert a.dtype == np.uint8
    flat = a if a.ndim == 3 else a[:, :, None]
    tmp = _pass_axis1(flat, size[1], filt)                                   # horizontal
    res = _pass_axis1(tmp.transpose(1, 0, 2), size[0], filt).transpose(1, 0, 2)   # vertical
    res = np.ascontiguousarray(res)
    return res if a.ndim == 3 else res[:, :, 0]


def pattern(h, w, c):
    """Closed-form test image (h, w, c) uint8 - (h, w) for c == 1: a quasi-texture plus a saturated block of 0s and 255s in
    its middle, which drives BICUBIC's negative lobes past both ends of the clamp.  The same bytes everywhere."""
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    img = ((7 * x + 13 * y + 29 * ch + (x * y) % 11) % 256).astype(np.uint8)
    y0, y1, x0, x1 = h // 4, max(h // 4 + 1, 3 * h // 4), w // 4, max(w // 4 + 1, 3 * w // 4)
    block = np.where(((x // 5 + y // 3) % 2) == 0, 0, 255).astype(np.uint8)
    img[y0:y1, x0:x1] = block[y0:y1, x0:x1]
    return img if c > 1 else img[:, :, 0]
