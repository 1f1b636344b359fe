"""numpy oracle of the view-consistency contract (include/wsdl_hip.h, "view consistency") - the yardstick of
csrc/consistency.hip, beside augment_oracle.py.  Two faces:

  * a FLOAT32 restatement of the warp: the coordinates are ``augment_oracle.source_coords`` (float32, every operation rounded on
    its own), the values the unfused float32 lerp ``top = v00 + fx * (v01 - v00)`` ... with the zero-fraction rule (a fraction
    of 0 takes its first tap as it is) - what the kernel computes, operation for operation; and float32 runs of the adjoint
    and of the loss, which are only the yardstick of the standing bound;
  * a FLOAT64 evaluation - warp values, the adjoint as ``np.add.at`` with the float32-derived taps and weights, the three
    loss kinds with their gradients - which everything is bounded against.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_oracle import F, source_coords  # noqa: E402

KINDS = ("kl", "mse", "hard")
ULP = 2.0 ** -23


def _index(f, add, hi):
    """float -> index of [0, hi]: brought into [-1, hi + 1] first (NaN -> -1), then ``+ add``, then clamped."""
    c = np.clip(np.nan_to_num(f, nan=-1.0, posinf=hi + 1.0, neginf=-1.0), -1.0, hi + 1.0).astype(np.int64) + add
    return np.clip(c, 0, hi)


def taps(row, src_hw, out_hw, fill="ignore"):
    """The float32 taps of one row: dict of inside (bool), fx, fy (float32), x0 x1 y0 y1 xl yl (int64), each (out_h, out_w)."""
    H, W = src_hw
    with np.errstate(all="ignore"):
        xs, ys, inside = source_coords(np.asarray(row, dtype=F), src_hw, out_hw, fill)
        inside = inside & np.isfinite(xs) & np.isfinite(ys)          # the added rule: a non-finite source point is outside
        xc, yc = xs - F(0.5), ys - F(0.5)
        x0f, y0f = np.floor(xc), np.floor(yc)
        fx, fy = (xc - x0f).astype(F), (yc - y0f).astype(F)
        return {"inside": inside, "fx": fx, "fy": fy,
                "x0": _index(x0f, 0, W - 1), "x1": _index(x0f, 1, W - 1), "y0": _index(y0f, 0, H - 1), "y1": _index(y0f, 1, H - 1),
                "xl": _index(np.floor(xs), 0, W - 1), "yl": _index(np.floor(ys), 0, H - 1)}


def _lerp(v00, v01, v10, v11, fx, fy):
    """The value rule in the dtype of its arguments, every operation rounded on its own; a zero fraction skips its lerp."""
    with np.errstate(all="ignore"):
        top = np.where(fx == 0, v00, v00 + fx * (v01 - v00))
        bot = np.where(fx == 0, v10, v10 + fx * (v11 - v10))
        return np.where(fy == 0, top, top + fy * (bot - top))


def warp_one(x, row, out_hw=None, fill="ignore", pad_value=0.0, photometric=False, dtype=np.float64):
    """x (C,h,w) float32 -> (values (C,out_h,out_w) in ``dtype``, inside).  ``dtype=float32`` is the kernel's arithmetic."""
    C, h, w = x.shape
    out_hw = (h, w) if out_hw is None else tuple(out_hw)
    t = taps(row, (h, w), out_hw, fill)
    xv = x.astype(dtype)
    fx, fy = t["fx"].astype(dtype), t["fy"].astype(dtype)
    val = _lerp(xv[:, t["y0"], t["x0"]], xv[:, t["y0"], t["x1"]], xv[:, t["y1"], t["x0"]], xv[:, t["y1"], t["x1"]], fx, fy)
    if photometric:
        with np.errstate(all="ignore"):
            val = dtype(F(row[6])) * val + dtype(F(row[7]))
    val = np.where(t["inside"][None], val, dtype(F(pad_value))).astype(dtype)
    return val, t["inside"]


def warp_scores(x, rows, out_hw=None, dtype=np.float64, **kw):
    """(B,C,h,w) -> (values (B,C,out_h,out_w), valid (B,out_h,out_w) uint8)."""
    outs = [warp_one(xb, row, out_hw, dtype=dtype, **kw) for xb, row in zip(np.asarray(x), np.asarray(rows, dtype=F))]
    return np.stack([o for o, _ in outs]), np.stack([v for _, v in outs]).astype(np.uint8)


def warp_labels(labels, rows, out_hw=None, fill="ignore", pad_label=-100):
    labels = np.asarray(labels)
    B, h, w = labels.shape
    out_hw = (h, w) if out_hw is None else tuple(out_hw)
    outs = []
    for lb, row in zip(labels, np.asarray(rows, dtype=F)):
        t = taps(row, (h, w), out_hw, fill)
        outs.append(np.where(t["inside"], lb[t["yl"], t["xl"]], np.int64(pad_label)))
    return np.stack(outs).astype(np.int64)


def adjoint_one(dy, row, src_hw, photometric=False, dtype=np.float64):
    """The adjoint of ``warp_one`` (fill = ignore) with respect to x: a scatter of dy (C,out_h,out_w) with the float32-derived
    taps and weights, accumulated in ``dtype`` by ``np.add.at``."""
    C, Ho, Wo = dy.shape
    h, w = src_hw
    t = taps(row, src_hw, (Ho, Wo), "ignore")
    m = t["inside"]
    fx, fy = t["fx"].astype(dtype)[m], t["fy"].astype(dtype)[m]
    g = dy.astype(dtype)[:, m]
    if photometric:
        g = g * dtype(F(row[6]))
    out = np.zeros((C, h, w), dtype=dtype)
    one = dtype(1)
    for ys, xs, wgt in ((t["y0"], t["x0"], (one - fx) * (one - fy)), (t["y0"], t["x1"], fx * (one - fy)),
                        (t["y1"], t["x0"], (one - fx) * fy), (t["y1"], t["x1"], fx * fy)):
        for c in range(C):
            np.add.at(out[c], (ys[m], xs[m]), wgt * g[c])
    return out


def adjoint(dy, rows, src_hw, dtype=np.float64, **kw):
    return np.stack([adjoint_one(d, row, src_hw, dtype=dtype, **kw) for d, row in zip(np.asarray(dy), np.asarray(rows, dtype=F))])


def pixel_terms(z, t, kind="kl", teacher_is="logits", temperature=1.0, dtype=np.float64):
    """Per pixel, in ``dtype``: z, t (B,C,H,W) (t already on the student's grid) -> dict of conf (B,H,W), target (B,H,W) int64,
    finite (B,H,W) bool, loss (B,H,W), grad (B,C,H,W) - the un-weighted loss term and its gradient with respect to z."""
    assert kind in KINDS and teacher_is in ("logits", "probs")
    with np.errstate(all="ignore"):
        z, t = z.astype(dtype), t.astype(dtype)
        C = z.shape[1]
        finite = np.isfinite(z).all(1) & np.isfinite(t).all(1)
        target = np.argmax(np.where(np.isnan(t), -np.inf, t), axis=1)           # the first class of largest teacher value
        dz = z - z.max(1, keepdims=True)
        ls = dz - np.log(np.exp(dz).sum(1, keepdims=True))
        s = np.exp(ls)
        if teacher_is == "logits":
            dt = (t - t.max(1, keepdims=True)) / dtype(F(temperature))
            lq = dt - np.log(np.exp(dt).sum(1, keepdims=True))
            q = np.exp(lq)
        else:
            tot = t.sum(1, keepdims=True)
            finite &= (t >= 0).all(1) & (tot[:, 0] > 0) & np.isfinite(tot[:, 0])
            q = t / tot
            lq = np.where(q > 0, np.log(np.where(q > 0, q, 1)), 0)
        conf = q.max(1)
        if kind == "kl":
            loss = (q * (lq - ls)).sum(1)
            grad = s - q
        elif kind == "mse":
            d = s - q
            loss = (d * d).sum(1) / dtype(C)
            grad = (dtype(2) / dtype(C)) * s * (d - (s * d).sum(1, keepdims=True))
        else:
            onehot = np.arange(C).reshape(1, C, 1, 1) == target[:, None]
            loss = -(ls * onehot).sum(1)
            grad = s - onehot.astype(dtype)
    return {"conf": conf, "target": target.astype(np.int64), "finite": finite, "loss": loss, "grad": grad}


def consistency(z, t, inside=None, *, kind="kl", teacher_is="logits", temperature=1.0, tau=0.0, lam=1.0, normalize="all",
                pixel_weight=None, weight=None, dtype=np.float64):
    """The loss and its gradient in ``dtype``.  ``inside`` (B,H,W) bool, default all.  ``weight``: the plane ``w`` to use (the
    device's published one) instead of the oracle's own decision ``counted * pixel_weight``.
    -> dict of loss (scalar), grad (B,C,H,W), weight (B,H,W), target, conf, counted, n_inside, n_counted."""
    terms = pixel_terms(z, t, kind, teacher_is, temperature, dtype)
    B, C, H, W = z.shape
    inside = np.ones((B, H, W), dtype=bool) if inside is None else np.asarray(inside).astype(bool)
    with np.errstate(all="ignore"):
        counted = inside & terms["finite"] & (terms["conf"] >= dtype(F(tau)))
    if weight is None:
        weight = counted.astype(dtype) * (1 if pixel_weight is None else np.asarray(pixel_weight).astype(dtype))
    weight = np.asarray(weight).astype(dtype)
    on = weight != 0
    N = dtype(B * H * W) if normalize == "all" else weight.sum(dtype=dtype)
    f = dtype(F(lam)) / N if N > 0 else dtype(0)
    loss = f * np.where(on, weight * np.where(on, terms["loss"], 0), 0).sum(dtype=dtype)
    grad = np.where(on[:, None], f * weight[:, None] * np.where(on[:, None], terms["grad"], 0), 0).astype(dtype)
    return {"loss": dtype(loss) if on.any() else dtype(0), "grad": grad, "weight": weight, "counted": counted,
            "target": np.where(counted, terms["target"], -100), "raw_target": terms["target"], "conf": terms["conf"],
            "n_inside": int(inside.sum()), "n_counted": int(counted.sum())}


# ---- the cases the CPU and the device tests share ---------------------------------------------------------------------------
GEOMS = ((1, 1, 1, 1), (1, 3, 1, 7), (1, 3, 7, 1), (2, 5, 5, 7), (3, 3, 37, 53), (2, 21, 64, 64), (2, 2, 96, 130), (1, 3, 3, 300),
         (1, 64, 9, 11))
ROW_NAMES = ("identity", "flip", "rot+30_x0.5", "rot-30_x2", "half_pixel", "outside", "nan", "singular")


def teacher_sizes(H, W):
    """The student's size, a smaller and a larger one."""
    return ((H, W), (max(1, (2 * H) // 3), max(1, W // 2 + 1)), (H + 3, 2 * W + 1))


def named_row(name, student_hw, teacher_hw):
    """One (8,) float32 row mapping the student's (output) grid onto the teacher's (source) grid."""
    from weaklysuperviseddl_amd.augment import affine_row
    (H, W), (h, w) = student_hw, teacher_hw
    if name == "identity":                  # (the plain resize where the sizes differ; 1 0 0 0 1 0 where they agree)
        return affine_row(0.0, (h, w), (H, W)).numpy()
    if name == "flip":
        return affine_row(0.0, (h, w), (H, W), flip=True).numpy()
    if name == "rot+30_x0.5":
        return affine_row(30.0, (h, w), (H, W), scale=0.5).numpy()
    if name == "rot-30_x2":
        return affine_row(-30.0, (h, w), (H, W), scale=2.0).numpy()
    if name == "half_pixel":                # fx = 0.5 exactly at equal sizes
        return np.array([w / W, 0, 0.5, 0, h / H, 0, 1, 0], dtype=F)
    if name == "outside":
        return np.array([1, 0, 1e6, 0, 1, 0, 1, 0], dtype=F)
    if name == "nan":
        return np.full(8, np.nan, dtype=F)
    assert name == "singular", name         # every output pixel reads the centre point: the adjoint's whole-output fallback
    return np.array([0, 0, w / 2, 0, 0, h / 2, 1, 0], dtype=F)


def row_batches(B, student_hw, teacher_hw):
    """The eight named rows dealt onto batches of B items (the last batch wraps around) -> list of (names, rows (B,8))."""
    out = []
    for k in range(0, len(ROW_NAMES), B):
        names = [ROW_NAMES[(k + j) % len(ROW_NAMES)] for j in range(B)]
        out.append((names, np.stack([named_row(n, student_hw, teacher_hw) for n in names]).astype(F)))
    return out


def loss_inputs(B, C, H, W, teacher_hw, seed, teacher_is="logits"):
    """Student logits ``randn`` and teacher logits ``3 * randn`` (or their softmax as probabilities), fixed seeds."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, C, H, W)).astype(F)
    t = (3.0 * rng.standard_normal((B, C) + tuple(teacher_hw))).astype(F)
    if teacher_is == "probs":
        e = np.exp(t.astype(np.float64) - t.max(1, keepdims=True))
        t = (e / e.sum(1, keepdims=True)).astype(F)
    return z, t


def near_tie(t32, t64, conf32, conf64, tau):
    """Pixels whose decision the float32 evaluation may legitimately take the other way: ``|conf - tau|`` or the gap between
    the two largest teacher values within twice the standing bound of that quantity."""
    bc = np.broadcast_to(bound(conf32, conf64), conf64.shape)
    near = np.abs(conf64 - np.float64(F(tau))) <= 2 * bc
    if t64.shape[1] > 1:
        top = np.sort(np.where(np.isfinite(t64), t64, -np.inf), axis=1)
        bt = np.broadcast_to(bound(t32, t64), t64.shape).max(1)
        with np.errstate(all="ignore"):
            near |= (top[:, -1] - top[:, -2]) <= 2 * bt
    return near


def bound(o32, o64, extra=0.0):
    """The project's standing bound, per element: max(4 x the float32 oracle's worst error of the tensor, 2^-23 |value|)."""
    o64 = np.asarray(o64, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(o32, dtype=np.float64) - o64)
        yard = float(np.nanmax(np.where(np.isfinite(d), d, 0.0))) if d.size else 0.0
    return np.maximum(4.0 * yard, ULP * np.abs(o64)) + extra


def ratio(got, o32, o64, extra=0.0):
    """Worst device error / bound over the finite elements of the float64 result (non-finite ones must match exactly)."""
    got, o64 = np.asarray(got, dtype=np.float64), np.asarray(o64, dtype=np.float64)
    fin = np.isfinite(o64)
    assert np.array_equal(got[~fin], o64[~fin], equal_nan=True)
    b = np.broadcast_to(bound(o32, o64, extra), o64.shape)
    err = np.abs(got - o64)[fin]
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(b[fin], 1e-300))))
