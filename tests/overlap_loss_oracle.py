"""Oracle of the overlap sums, the Tversky / soft Dice loss with its gradient and the focal loss with its gradient
(include/wsdl_hip.h "overlap and focal losses"), written from the contract in torch on the CPU.

Everything exists in float64 and in float32: the float32 run - every operation in torch float32, from the float32 logits -
against the float64 run is the yardstick of the device tests.  The gradients are written out in closed form, not taken from
autograd; tests/test_overlap_loss.py compares them with autograd of the direct definitions.

Definitions.  s = softmax(logits) over C; a pixel is valid when labels != ignore_index; segments are the images with
``per_image``, else the batch; y_c = 1 where the pixel is valid and labels == c.  Per segment and listed class:
I = sum s_c y_c, P = sum_valid s_c, Y = sum y_c; N = I + smooth, D = I + alpha (P - I) + beta (Y - I) + smooth; T = N / D, 1 where
D == 0; term = (1 - T)^gamma, exactly 0 with a zero gradient where 1 - T <= 0; ``present_only`` drops the classes with Y == 0
in their segment; loss = scale x mean of the kept terms, 0 without one.  Focal: l = p w[y] q^gamma (-log s_y) with q = 1 - s_y
formed as the sum of the other classes' probabilities."""
import torch

IGNORE = 255

# (B, C, H, W) of the device tests: one pixel; a scalar tail; C == 3 in registers at an odd size; the general case; the
# generic-C vector path; several workgroups per image (96 x 130 / 4 = 3120 items: 13 workgroups), so the fixed-order
# finalize matters; a row wider than a workgroup
SHAPES = ((1, 2, 1, 1), (1, 2, 1, 7), (2, 3, 5, 7), (3, 3, 37, 53), (2, 21, 64, 64), (2, 2, 96, 130), (1, 3, 3, 300))
TVERSKY = ((0.5, 0.5, 1.0), (0.3, 0.7, 0.75), (0.7, 0.3, 2.0))
CLASS_LISTS = (None, (1,), (2, 0))


def make_logits(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(B, C, H, W, generator=g)).contiguous()


def make_labels(B, C, H, W, seed, ignore=IGNORE):
    """Random labels in [0, C) with a strip of ``ignore`` (the last column group of every image; a single pixel stays valid)."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (B, H, W), generator=g)
    if H * W > 1:
        labels[:, : max(1, H // 3), W - max(1, W // 4):] = ignore
    return labels


def one_hot(labels, classes, ignore_index, dtype):
    """(B,K,H,W): y_c of the listed classes; (B,H,W): the valid pixels."""
    valid = labels != ignore_index
    y = torch.stack([(labels == c) & valid for c in classes], dim=1)
    return y.to(dtype), valid.to(dtype)


def overlap_sums(logits, labels, classes=None, ignore_index=-100, per_image=False, dtype=torch.float64):
    """(segments, K, 3) in ``dtype``: I, P, Y."""
    z = logits.to(dtype)
    C = z.shape[1]
    classes = tuple(range(C)) if classes is None else tuple(classes)
    s = torch.softmax(z, dim=1)[:, list(classes)]
    y, valid = one_hot(labels, classes, ignore_index, dtype)
    dims = (2, 3) if per_image else (0, 2, 3)
    I = (s * y).sum(dim=dims)
    P = (s * valid[:, None]).sum(dim=dims)
    Y = y.sum(dim=dims)
    out = torch.stack([I, P, Y], dim=-1)
    return out if per_image else out[None]


def tversky_from_sums(sums, alpha, beta, gamma, smooth, present_only, scale):
    """(loss, a, b) from (S,K,3) sums in their dtype: the terms, their mean and the gradient coefficients
    d loss / d s_c(p) = a y_c(p) + b at valid pixels."""
    dtype = sums.dtype
    I, P, Y = sums[..., 0], sums[..., 1], sums[..., 2]
    N = I + smooth
    D = I + alpha * (P - I) + beta * (Y - I) + smooth
    safe = torch.where(D == 0, torch.ones_like(D), D)
    T = torch.where(D == 0, torch.ones_like(D), N / safe)
    u = 1.0 - T
    live = u > 0
    up = torch.where(live, u, torch.ones_like(u))
    term = torch.where(live, up ** gamma, torch.zeros_like(u))
    kept = torch.ones_like(live) if not present_only else Y != 0
    n = int(kept.sum())
    if n == 0:
        return torch.zeros((), dtype=dtype), torch.zeros_like(I), torch.zeros_like(I)
    scale = torch.as_tensor(scale, dtype=dtype)
    loss = scale * ((term * kept.to(dtype)).sum() / n)
    w = scale * gamma * up ** (gamma - 1.0) / n
    on = (live & kept & (D != 0)).to(dtype)
    b = on * w * N * alpha / (safe * safe)
    a = -on * w * (safe - N * (1.0 - alpha - beta)) / (safe * safe)
    return loss, a, b


def tversky(logits, labels, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False,
            ignore_index=-100, scale=1.0, dtype=torch.float64):
    """(loss, grad) in ``dtype``; grad = d loss / d logits = s_j (g_j - sum_c s_c g_c) with g_c = a_c y_c + b_c for the listed
    classes and 0 for the others, exactly 0 at invalid pixels."""
    z = logits.to(dtype)
    B, C, H, W = z.shape
    classes = tuple(range(C)) if classes is None else tuple(classes)
    sums = overlap_sums(z, labels, classes, ignore_index, per_image, dtype)
    loss, a, b = tversky_from_sums(sums, alpha, beta, gamma, smooth, present_only, scale)
    s = torch.softmax(z, dim=1)
    y, valid = one_hot(labels, classes, ignore_index, dtype)
    if not per_image:
        a, b = a.expand(B, -1), b.expand(B, -1)
    g = torch.zeros_like(z)
    for k, c in enumerate(classes):
        g[:, c] = a[:, k, None, None] * y[:, k] + b[:, k, None, None]
    dot = (s * g).sum(dim=1, keepdim=True)
    grad = s * (g - dot) * valid[:, None]
    return loss, grad


def dice(logits, labels, smooth=1.0, **kw):
    return tversky(logits, labels, 0.5, 0.5, 1.0, smooth / 2.0, **kw)


def focal(logits, labels, gamma=2.0, weight=None, ignore_index=-100, reduction="mean", pixel_weight=None, dtype=torch.float64):
    """(loss, grad) in ``dtype``: grad is the gradient of the REDUCED loss ('none': of the sum of the map, i.e. each pixel's
    own gradient).  A label outside [0, C) other than ``ignore_index`` gives NaN at that pixel."""
    z = logits.to(dtype)
    B, C, H, W = z.shape
    p = torch.ones(B, H, W, dtype=dtype) if pixel_weight is None else pixel_weight.to(dtype)
    ignored = (labels == ignore_index) | (p == 0)
    bad = ~ignored & ((labels < 0) | (labels >= C))
    lab = torch.where(ignored | bad, torch.zeros_like(labels), labels)
    hot = torch.zeros(B, C, H, W, dtype=torch.bool).scatter_(1, lab[:, None], True)
    m = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - m)
    se = e.sum(dim=1)
    s = e / se[:, None]
    so = (e * (~hot).to(dtype)).sum(dim=1)               # the other classes' exponentials
    q = so / se                                           # 1 - s_y, without the subtraction
    dy = ((z - m) * hot.to(dtype)).sum(dim=1)
    sy = (e * hot.to(dtype)).sum(dim=1) / se
    nls = torch.where(dy == 0, torch.log1p(so), torch.log(se) - dy)      # -log s_y
    gam = torch.as_tensor(gamma, dtype=dtype)
    qg = torch.ones_like(q) if gamma == 0 else q ** gam
    ratio = torch.where(q == 0, -torch.ones_like(q), -nls / torch.where(q == 0, torch.ones_like(q), q))
    factor = qg * (gam * sy * ratio - 1.0)                # gamma s_y q^(gamma-1) log s_y - q^gamma
    w = torch.ones(C, dtype=dtype) if weight is None else weight.to(dtype)
    live = (~ignored & ~bad).to(dtype)
    wy = p * w[lab] * live
    l = wy * qg * nls
    coef = -wy * factor
    grad = torch.where(hot, -(coef * q)[:, None], coef[:, None] * s)
    nan = torch.full_like(l, float("nan"))
    l = torch.where(bad, nan, l)
    grad = torch.where(bad[:, None], nan[:, None].expand_as(grad), grad)
    grad = torch.where(ignored[:, None], torch.zeros_like(grad), grad)
    if reduction == "none":
        return l, grad
    if reduction == "sum":
        return l.sum(), grad
    den = wy.sum()
    return l.sum() / den, grad / den
