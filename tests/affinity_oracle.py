"""CPU oracle of the AffinityNet ops (include/wsdl_hip.h "AffinityNet"; Ahn & Kwak, CVPR 2018): vectorised torch with a ``dtype``
argument - float64 is the reference, the same code in float32 the yardstick of the parity bound.

Pairs: PSA's half disc; a pair (p, q = p + o_j) is valid iff q lies inside the image (not PSA's crop of the "from" region).
Everything is written with shifted slices; ``dense_transition_matrix`` / ``dense_walk`` are PSA's own formulation - the dense
``(A + I) ** beta`` matrix, column-normalised, raised to a power - and exist to check the stencil walk against it."""
import torch

# (B, D, h, w)
CASES = (
    (1, 1, 1, 1),          # no valid pair at all
    (1, 3, 1, 7),
    (1, 3, 7, 1),
    (2, 5, 5, 7),          # at radius 8 every offset is longer than one side
    (2, 448, 9, 11),       # the channel-chunk loop
    (1, 64, 33, 65),       # tile seams and ragged edges
    (2, 7, 64, 64),
    (1, 4, 70, 70),        # beyond any single-workgroup path
)
RADII = (2, 5, 8)
# (case, radius, beta, C): every shape, every radius, both betas, C = 1, 2 and 21
WALK_CASES = (
    (0, 2, 8.0, 1),
    (1, 5, 1.0, 2),
    (2, 2, 8.0, 2),
    (3, 8, 8.0, 21),
    (3, 5, 1.0, 1),
    (4, 5, 8.0, 2),
    (5, 5, 1.0, 21),
    (5, 8, 8.0, 1),
    (6, 5, 8.0, 2),
    (6, 2, 1.0, 21),
    (7, 2, 8.0, 1),
    (7, 5, 8.0, 2),
)
WALK_STEPS = (1, 16, 256)


def offsets(radius):
    out = [(0, x) for x in range(1, radius)]
    out += [(y, x) for y in range(1, radius) for x in range(-(radius - 1), radius) if x * x + y * y < radius * radius]
    return out


def window(h, w, dy, dx):
    """Slices (from-rows, from-cols, to-rows, to-cols) of the pixels p whose partner p + (dy, dx) is inside an h x w image; None
    when there is none.  dy >= 0."""
    y1 = h - dy
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y1 <= 0 or x1 <= x0:
        return None
    return slice(0, y1), slice(x0, x1), slice(dy, y1 + dy), slice(x0 + dx, x1 + dx)


def make_features(B, D, h, w, seed):
    """Smooth-ish features with per-channel structure: neighbours are related, distant pixels are not."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, D, h, w, generator=g)
    if h > 1:
        base[:, :, 1:] = 0.6 * base[:, :, 1:] + 0.4 * base[:, :, :-1]
    if w > 1:
        base[:, :, :, 1:] = 0.6 * base[:, :, :, 1:] + 0.4 * base[:, :, :, :-1]
    return (base * 1.5).float()


def make_labels(B, h, w, seed, variant="all"):
    """int64 labels in coarse blocks.  'all': 0, 1, 2 and 255 - all three pair kinds (where the image has room for them);
    'no_bg': 1, 2 and 255 - no bg-positive pair; 'ignored': 255 everywhere."""
    g = torch.Generator().manual_seed(seed)
    if variant == "ignored":
        return torch.full((B, h, w), 255, dtype=torch.int64)
    values = torch.tensor([0, 1, 2, 255] if variant == "all" else [1, 2, 255, 1])
    coarse = torch.randint(0, 4, (B, (h + 2) // 3, (w + 2) // 3), generator=g)
    first = min(4, coarse[0].numel())
    coarse.view(B, -1)[:, :first] = torch.arange(first)            # (every value occurs where the image has room for it)
    lab = values[coarse].repeat_interleave(3, dim=1).repeat_interleave(3, dim=2)[:, :h, :w]
    return lab.contiguous()


def make_scores(B, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, h, w, generator=g)


def affinity(feat, radius, dtype=torch.float64):
    """(B,P,h,w): exp(-mean_d |f_d(p) - f_d(p + o_j)|), 0 at an invalid pair.  Differentiable."""
    f = feat.to(dtype)
    B, D, h, w = f.shape
    offs = offsets(radius)
    out = torch.zeros(B, len(offs), h, w, dtype=dtype)
    for j, (dy, dx) in enumerate(offs):
        win = window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        out[:, j, ys, xs] = torch.exp(-(f[:, :, ys, xs] - f[:, :, yt, xt]).abs().mean(dim=1))
    return out


def pair_kinds(labels, radius, ignore_index=255):
    """bool (3,B,P,h,w): bg-positive, fg-positive, negative."""
    B, h, w = labels.shape
    offs = offsets(radius)
    kinds = torch.zeros(3, B, len(offs), h, w, dtype=torch.bool)
    for j, (dy, dx) in enumerate(offs):
        win = window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        a, b = labels[:, ys, xs], labels[:, yt, xt]
        ok = (a != ignore_index) & (b != ignore_index)
        kinds[0, :, j, ys, xs] = ok & (a == b) & (a == 0)
        kinds[1, :, j, ys, xs] = ok & (a == b) & (a > 0)
        kinds[2, :, j, ys, xs] = ok & (a != b)
    return kinds


def pair_counts(labels, radius, ignore_index=255):
    return pair_kinds(labels, radius, ignore_index).flatten(1).sum(dim=1)


def loss_from_affinity(aff, kinds, weights=(0.25, 0.25, 0.5), eps=1e-5):
    """PSA's train_aff loss from affinities (any device): the form the device's autograd test uses too."""
    n = kinds.flatten(1).sum(dim=1).to(aff.dtype)
    k = kinds.to(aff.dtype)
    terms = (-(torch.log(aff + eps)) * k[0]).sum() / (n[0] + eps), (-(torch.log(aff + eps)) * k[1]).sum() / (n[1] + eps), \
        (-(torch.log(1.0 + eps - aff)) * k[2]).sum() / (n[2] + eps)
    return weights[0] * terms[0] + weights[1] * terms[1] + weights[2] * terms[2]


def loss(feat, labels, radius, ignore_index=255, weights=(0.25, 0.25, 0.5), eps=1e-5, dtype=torch.float64):
    """(loss, dL/dfeat) by torch autograd of the slice formulation."""
    f = feat.detach().to(dtype).requires_grad_()
    L = loss_from_affinity(affinity(f, radius, dtype), pair_kinds(labels, radius, ignore_index), weights, eps)
    if L.requires_grad:
        L.backward()
    grad = f.grad if f.grad is not None else torch.zeros_like(f)
    return L.detach(), grad.detach()


def transitions(aff, beta, radius):
    """(B,2P+1,h,w) in aff's dtype: plane 0 self, 1 + 2j the neighbour at o_j, 2 + 2j the one at -o_j; rows sum to 1."""
    B, P, h, w = aff.shape
    offs = offsets(radius)
    pw = torch.zeros(B, 2 * P + 1, h, w, dtype=aff.dtype)
    pw[:, 0] = 1
    for j, (dy, dx) in enumerate(offs):
        win = window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        v = aff[:, j, ys, xs] ** beta
        pw[:, 1 + 2 * j, ys, xs] = v
        pw[:, 2 + 2 * j, yt, xt] = v
    return pw / pw.sum(dim=1, keepdim=True)


def walk_step(trans, m, radius):
    B, C, h, w = m.shape
    out = trans[:, 0:1] * m
    for j, (dy, dx) in enumerate(offsets(radius)):
        win = window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        out[:, :, ys, xs] += trans[:, 1 + 2 * j:2 + 2 * j, ys, xs] * m[:, :, yt, xt]
        out[:, :, yt, xt] += trans[:, 2 + 2 * j:3 + 2 * j, yt, xt] * m[:, :, ys, xs]
    return out


def walk(trans, scores, steps, radius):
    """The stencil walk: {n: scores after n steps} for the step counts in ``steps``, in trans's dtype."""
    m = scores.to(trans.dtype).clone()
    out = {}
    for it in range(max(steps) + 1):
        if it in steps:
            out[it] = m.clone()
        if it < max(steps):
            m = walk_step(trans, m, radius)
    return out


def dense_transition_matrix(aff, beta, radius):
    """PSA's matrix for ONE image (aff (1,P,h,w)): A symmetric with the pair affinities, T = (A + I) ** beta (elementwise),
    every column divided by its sum."""
    _, P, h, w = aff.shape
    n = h * w
    A = torch.zeros(n, n, dtype=aff.dtype)
    idx = torch.arange(n).view(h, w)
    for j, (dy, dx) in enumerate(offsets(radius)):
        win = window(h, w, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        p, q = idx[ys, xs].reshape(-1), idx[yt, xt].reshape(-1)
        A[p, q] = aff[0, j, ys, xs].reshape(-1)
        A[q, p] = aff[0, j, ys, xs].reshape(-1)
    T = (A + torch.eye(n, dtype=aff.dtype)) ** beta
    return T / T.sum(dim=0, keepdim=True)


def dense_walk(aff, scores, beta, num_iter, radius):
    """PSA's ``cam @ T^t`` for one image: scores (1,C,h,w)."""
    _, C, h, w = scores.shape
    T = dense_transition_matrix(aff, beta, radius)
    return (scores.to(aff.dtype).view(C, h * w) @ torch.linalg.matrix_power(T, num_iter)).view(1, C, h, w)
