"""Oracle of the prototype ops (csrc/prototype.hip; include/wsdl_hip.h "Class prototypes") in plain torch on the CPU, in float64
or - the yardstick of the device tests - in float32: the same statements, evaluated in ``dtype``.  tests/test_prototype.py holds
it to independent formulations (F.normalize + einsum + F.cross_entropy under autograd, per-pixel loops, central differences).

Definitions.  n(x) = max(sqrt(sum_d x_d^2), eps), u_p = f_p / n(f_p).  A segment is one image (S = B) or the batch (S = 1).
mass[s,k] = sum of w_p over the segment's pixels with label k (labels equal to ignore_index or outside [0,K) are not pooled);
proto[s,k] = sum w_p x_p / mass[s,k] with x_p = u_p (normalize) or f_p, exactly 0 where the mass is 0.  sim[b,k,p] = <u_p, q_k>,
q_k = proto[s(b),k] / n(proto[s(b),k]).  Contrast: z = sim / temperature over the present classes, l_p = -log softmax(z_p)[y_p];
a pixel counts iff its label is not ignore_index and its class is present; a label outside [0,K) other than ignore_index gives
NaN; the prototypes are constants."""
import torch

# (B, D, h, w): the smallest shapes at which each kernel can still go wrong - the minimum, a single row / column, a small odd map,
# AffinityNet's channel count, every chunk of 64 channels and the largest D, ragged lanes, full tiles of 64 pixels, ragged tiles
CASES = ((1, 1, 1, 1), (1, 3, 1, 7), (1, 3, 7, 1), (2, 5, 5, 7), (2, 448, 9, 11), (1, 2048, 3, 5), (1, 64, 33, 65), (2, 7, 64, 64),
         (1, 4, 70, 70))
CLASS_COUNTS = (1, 2, 3, 21, 32)                    # both sides of every bucket of the compiled class count
TEMPERATURES = (0.07, 0.1, 1.0)
OFFSETS = ((0.0, 1.0), (100.0, 1.0))                # (offset, scale) of the features
IGNORE = 255


def make_features(B, D, h, w, seed, offset=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, D, h, w, generator=g) * scale + offset).float()


def make_labels(B, h, w, K, seed, variant="all"):
    """int64 labels in [0, K) with about a tenth ignored.  'absent': class K - 1 does not occur in image 0; 'ignored': everything is
    ignored."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, K, (B, h, w), generator=g)
    lab[torch.rand(B, h, w, generator=g) < 0.1] = IGNORE
    if variant == "absent":
        lab[0][lab[0] == K - 1] = 0 if K > 1 else IGNORE
    elif variant == "ignored":
        lab[:] = IGNORE
    return lab


def make_weights(B, h, w, seed):
    """Pixel weights in [0, 2) with about a fifth exactly 0."""
    g = torch.Generator().manual_seed(seed)
    pw = torch.rand(B, h, w, generator=g) * 2
    pw[torch.rand(B, h, w, generator=g) < 0.2] = 0.0
    return pw.float()


def norm(x, eps, dim):
    return x.pow(2).sum(dim=dim, keepdim=True).sqrt().clamp_min(eps)


def prototypes(feat, labels, K, pixel_weight=None, per_image=True, normalize=True, ignore_index=IGNORE, eps=1e-12, dtype=torch.float64):
    f = feat.to(dtype)
    x = f / norm(f, eps, 1) if normalize else f
    B, D = f.shape[:2]
    w = torch.ones(labels.shape, dtype=dtype) if pixel_weight is None else pixel_weight.to(dtype)
    S = B if per_image else 1
    proto, mass = torch.zeros(S, K, D, dtype=dtype), torch.zeros(S, K, dtype=dtype)
    for k in range(K):
        if k == ignore_index:
            continue
        m = (labels == k).to(dtype) * w
        num, ms = (x * m[:, None]).sum(dim=(2, 3)), m.sum(dim=(1, 2))
        if not per_image:
            num, ms = num.sum(dim=0, keepdim=True), ms.sum(dim=0, keepdim=True)
        mass[:, k] = ms
        proto[:, k] = torch.where(ms[:, None] > 0, num / ms.clamp_min(torch.finfo(dtype).tiny)[:, None], torch.zeros_like(num))
    return proto, mass


def _per_image(t, B):
    return t.expand(B, *t.shape[1:]) if t.shape[0] != B else t


def _present(present, B, K):
    if present is None:
        return torch.ones(B, K, dtype=torch.bool)
    return _per_image(present.bool(), B)


def cosine(feat, proto, eps=1e-12, dtype=torch.float64):
    f, q = feat.to(dtype), proto.to(dtype)
    u, q = f / norm(f, eps, 1), q / norm(q, eps, 2)
    return torch.einsum("bdhw,bkd->bkhw", u, _per_image(q, f.shape[0]))


def similarity(feat, proto, activation="none", temperature=1.0, present=None, eps=1e-12, dtype=torch.float64):
    sim = cosine(feat, proto, eps, dtype)
    if activation == "none":
        return sim
    if activation == "relu":
        return sim.clamp_min(0)
    on = _present(present, sim.shape[0], sim.shape[1])[:, :, None, None].expand_as(sim)
    z = torch.where(on, sim / temperature, torch.full_like(sim, -float("inf")))
    m = z.amax(dim=1, keepdim=True)
    e = torch.where(on, (z - torch.where(torch.isfinite(m), m, torch.zeros_like(m))).exp(), torch.zeros_like(z))
    s = e.sum(dim=1, keepdim=True)
    return torch.where(on, e / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(e))


def contrast(feat, proto, labels, temperature=0.1, present=None, pixel_weight=None, ignore_index=IGNORE, reduction="mean", eps=1e-12,
             dtype=torch.float64):
    """(loss, dloss / dfeat) by the closed form; for 'none' the gradient is that of the SUM of the per-pixel losses."""
    f, q = feat.to(dtype), proto.to(dtype)
    B, D, h, w_ = f.shape
    K = q.shape[1]
    raw = f.pow(2).sum(dim=1, keepdim=True).sqrt()
    clamped = raw < eps
    n = torch.where(clamped, torch.full_like(raw, eps), raw)
    u = f / n
    q = _per_image(q / norm(q, eps, 2), B)
    sim = torch.einsum("bdhw,bkd->bkhw", u, q)
    on = _present(present, B, K)
    in_range = (labels >= 0) & (labels < K)
    y = torch.where(in_range, labels, torch.zeros_like(labels))
    counted = (labels != ignore_index) & in_range & torch.gather(on, 1, y.reshape(B, -1)).reshape(B, h, w_)
    bad = (labels != ignore_index) & ~in_range
    w = torch.ones(labels.shape, dtype=dtype) if pixel_weight is None else pixel_weight.to(dtype)
    p = similarity(feat, proto, "softmax", temperature, present, eps, dtype)
    onehot = torch.zeros_like(p).scatter_(1, y[:, None], 1.0)
    py = (p * onehot).sum(dim=1)
    l = torch.where(counted, -torch.where(counted, py, torch.ones_like(py)).log(), torch.zeros_like(py)) * w
    l = torch.where(bad, torch.full_like(l, float("nan")), l)
    g = torch.where(counted[:, None], (p - onehot) * w[:, None], torch.zeros_like(p))
    total = (w * counted).sum()
    if reduction == "mean":
        scale = 1.0 / total if total > 0 else torch.zeros((), dtype=dtype)
        loss = l.sum() * scale if total > 0 else (l.sum() * 0 if not bad.any() else l.sum())
        g = g * scale
    else:
        loss = l.sum() if reduction == "sum" else l
    v = torch.einsum("bkhw,bkd->bdhw", g, q) / temperature
    c = (g * sim).sum(dim=1, keepdim=True) / temperature
    grad = torch.where(clamped, v / eps, (v - c * u) / n)
    grad = torch.where(bad[:, None], torch.full_like(grad, float("nan")), grad)
    return loss, grad


def ema(bank, count, proto, mass, momentum):
    """(bank, count) after one update, in float64."""
    bank, proto = bank.double().clone(), proto.double().reshape(bank.shape)
    count, mass = count.clone(), mass.reshape(-1)
    for k in range(bank.shape[0]):
        if mass[k] > 0:
            bank[k] = proto[k] if count[k] == 0 else momentum * bank[k] + (1 - momentum) * proto[k]
            count[k] += 1
    return bank, count
