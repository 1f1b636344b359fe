"""GroupNorm restated in plain torch ops, generic in the dtype: the float64 run is the reference of tests/test_hip_group_norm.py,
the float32 run its yardstick.

Two passes, as the definition reads: the mean of a group, then the centred second moment about that mean (biased).  The backward
is the closed form; it takes the ReLU mask as an ARGUMENT, so the same formula can be evaluated with the mask a float64 forward
gives, with the mask a float32 forward gives or with the mask the device wrote."""
import torch

# (B, C, H, W, G): the smallest shapes at which the kernels of csrc/group_norm.hip can still go wrong
CASES = (
    (1, 1, 1, 1, 1),        # one element
    (1, 4, 1, 7, 2),        # odd HW: one float per lane
    (2, 6, 5, 7, 3),        # small odd geometry
    (1, 8, 3, 300, 8),      # C / G = 1
    (2, 12, 96, 130, 1),    # one group per image, the largest n; float4 path, seven chunks per plane, the last one short
    (2, 160, 9, 11, 32),    # many channels, tiny planes
    (3, 32, 37, 53, 4),     # IRN's head shape, odd planes
    (2, 32, 64, 64, 4),     # IRN's head at a 256 x 256 image; float4 path, two full chunks per plane
    (1, 2, 45, 47, 1),      # odd HW above one chunk: the one-float-per-lane path with two chunks per plane
)
# offset, scale of the data
CONTENTS = ((0.0, 1.0), (100.0, 1.0), (-1000.0, 0.5))


def name_of(case):
    return "x".join(str(v) for v in CASES[case][:4]) + f" G={CASES[case][4]}"


def make_inputs(case, content, seed=0):
    """x, gamma, beta and the upstream gradient of one case, float32, from a seeded generator."""
    B, C, H, W, G = CASES[case]
    offset, scale = CONTENTS[content]
    g = torch.Generator().manual_seed(1000 * seed + 10 * case + content)
    x = torch.randn(B, C, H, W, generator=g) * scale + offset
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g) * 0.5
    dy = torch.randn(B, C, H, W, generator=g)
    return x, gamma, beta, dy


def _grouped(t, G):
    return t.reshape(t.shape[0], G, -1)


def forward(x, G, gamma=None, beta=None, eps=1e-5, relu=False, dtype=torch.float64):
    """-> y, pre (the value in front of the ReLU; y itself without relu), mean (B,G), rstd (B,G), all in ``dtype``."""
    x = x.to(dtype)
    B, C = x.shape[0], x.shape[1]
    xg = _grouped(x, G)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = ((xg - mean) * rstd).reshape(x.shape)
    shape = (1, C) + (1,) * (x.dim() - 2)
    if gamma is not None:
        pre = pre * gamma.to(dtype).view(shape)
    if beta is not None:
        pre = pre + beta.to(dtype).view(shape)
    y = torch.clamp(pre, min=0) if relu else pre
    return y, pre, mean[:, :, 0], rstd[:, :, 0]


def backward(x, dy, G, gamma=None, eps=1e-5, mask=None, dtype=torch.float64):
    """The closed form, with ``mask`` (like x, or None for no ReLU) multiplied into the upstream gradient:
    dx = rstd (g - mean_grp(g) - xhat mean_grp(g xhat)) with g = dy m gamma, dgamma = sum dy m xhat, dbeta = sum dy m."""
    x, dy = x.to(dtype), dy.to(dtype)
    B, C = x.shape[0], x.shape[1]
    xg = _grouped(x, G)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((xg - mean) * rstd).reshape(x.shape)
    dym = dy if mask is None else dy * mask.to(dtype)
    shape = (1, C) + (1,) * (x.dim() - 2)
    g = dym if gamma is None else dym * gamma.to(dtype).view(shape)
    gg, xh = _grouped(g, G), _grouped(xhat, G)
    dx = (rstd * (gg - gg.mean(dim=2, keepdim=True) - xh * (gg * xh).mean(dim=2, keepdim=True))).reshape(x.shape)
    dims = [0] + list(range(2, x.dim()))
    return dx, (dym * xhat).sum(dim=dims), dym.sum(dim=dims)
