"""numpy restatement of the augmentation contract (include/wsdl_hip.h, "joint image / label augmentation") - the oracle of
csrc/augment.hip, beside pil_resize_oracle.py.

The COORDINATES are float32 exactly as the contract writes them - every operation an element-wise numpy float32 operation,
which rounds once and never contracts - so the oracle selects the source pixels the kernel selects.  The interpolation and
``gain * value + bias`` run in float64: the yardstick the kernel's float32 values are bounded against.
"""
import numpy as np

F = np.float32
IDENTITY = (1, 0, 0, 0, 1, 0, 1, 0)


def _reflect(s, n):
    P = F(2) * F(n)
    q = np.floor(s / P)
    r = s - P * q
    r = np.where(r < 0, r + P, r)
    r = np.where(r >= F(n), P - r, r)
    return r.astype(F)


def source_coords(row, src_hw, out_hw, fill):
    """(xs, ys, inside) of one parameter row, each (out_h, out_w); xs / ys float32."""
    H, W = src_hw
    Ho, Wo = out_hw
    a00, a01, a02, a10, a11, a12 = (F(v) for v in row[:6])
    u = (np.arange(Wo, dtype=F) + F(0.5))[None, :]
    v = (np.arange(Ho, dtype=F) + F(0.5))[:, None]
    xs = ((a00 * u + a01 * v) + a02).astype(F)
    ys = ((a10 * u + a11 * v) + a12).astype(F)
    assert xs.dtype == F and ys.dtype == F
    if fill == "reflect":
        xs, ys = _reflect(xs, W), _reflect(ys, H)
        inside = np.ones((Ho, Wo), dtype=bool)
    else:
        assert fill == "ignore", fill
        inside = (xs >= 0) & (xs < F(W)) & (ys >= 0) & (ys < F(H))
    return xs, ys, inside


def augment_one(image, label, row, out_hw, fill="ignore", pad_value=0.0, pad_label=-100, label_lut=None):
    """image (C,H,W) float (already through any uint8 table), label (H,W) uint8, row: 8 values ->
    (image_out (C,out_h,out_w) float64, label_out (out_h,out_w) int64)."""
    C, H, W = image.shape
    xs, ys, inside = source_coords(row, (H, W), out_hw, fill)
    # label: nearest
    xl = np.clip(np.floor(xs).astype(np.int64), 0, W - 1)
    yl = np.clip(np.floor(ys).astype(np.int64), 0, H - 1)
    raw = label[yl, xl]
    mapped = raw.astype(np.int64) if label_lut is None else np.asarray(label_lut, dtype=np.int64)[raw]
    label_out = np.where(inside, mapped, np.int64(pad_label))
    # image: four clamped taps
    xc, yc = xs - F(0.5), ys - F(0.5)
    x0f, y0f = np.floor(xc), np.floor(yc)
    fx, fy = (xc - x0f).astype(F), (yc - y0f).astype(F)
    assert fx.dtype == F and fy.dtype == F
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    img = image.astype(np.float64)
    fx64, fy64 = fx.astype(np.float64), fy.astype(np.float64)
    v00, v01, v10, v11 = img[:, ya, xa], img[:, ya, xb], img[:, yb, xa], img[:, yb, xb]
    top = v00 + fx64 * (v01 - v00)
    bot = v10 + fx64 * (v11 - v10)
    val = top + fy64 * (bot - top)
    gain, bias = np.float64(F(row[6])), np.float64(F(row[7]))
    image_out = np.where(inside[None], gain * val + bias, np.float64(F(pad_value)))
    return image_out, label_out


def augment_batch(images, labels, idx, params, out_hw=None, lut=None, label_lut=None, fill="ignore", pad_value=0.0,
                  pad_label=-100):
    """The batched call of ``ops.augment_batch`` on numpy arrays: images (N,C,H,W) float or uint8 (with lut (C,256)),
    labels (N,H,W) uint8, idx (B,), params (B,8)."""
    images, labels = np.asarray(images), np.asarray(labels)
    N, C, H, W = images.shape
    out_hw = (H, W) if out_hw is None else tuple(out_hw)
    outs, labs = [], []
    for n, row in zip(np.asarray(idx), np.asarray(params, dtype=F)):
        img = images[n]
        if images.dtype == np.uint8:
            img = np.stack([np.asarray(lut, dtype=F)[c][img[c]] for c in range(C)])
        o, l = augment_one(img, labels[n], row, out_hw, fill, pad_value, pad_label, label_lut)
        outs.append(o)
        labs.append(l)
    return np.stack(outs), np.stack(labs)
