"""Oracle of pixel-adaptive mask refinement (include/wsdl_hip.h "PAMR"; Araslanov & Roth, CVPR 2020), written from the
contract by clamped index gathers in torch.  The arithmetic runs in the dtype of ``dtype`` (default float64): the float64
run is the reference of the parity tests, the float32 run of the same code on the CPU is their yardstick.

Neighbourhood: for each dilation d, in the order given, the offsets (dy d, dx d) with dy, dx in {-1,0,1} in raster order
without the centre - P = 8 D neighbours; borders are replicated, every coordinate clamped on its own."""
import torch

DILATIONS = (1, 2, 4, 8, 12, 24)


def offsets(dilations=DILATIONS):
    """[(oy, ox)] of the P = 8 D neighbours, in plane order."""
    return [(dy * d, dx * d) for d in dilations for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def gather(t, oy, ox):
    """t (..., H, W) -> t at (clamp(y + oy), clamp(x + ox))."""
    H, W = t.shape[-2:]
    iy = (torch.arange(H) + oy).clamp(0, H - 1)
    ix = (torch.arange(W) + ox).clamp(0, W - 1)
    return t[..., iy, :][..., ix]


def neighbours(t, dilations=DILATIONS):
    """t (B,C,H,W) -> (B,C,P,H,W)."""
    return torch.stack([gather(t, oy, ox) for oy, ox in offsets(dilations)], dim=2)


def affinity(images, dilations=DILATIONS, dtype=torch.float64):
    """images (B,K,H,W) -> weights (B,P,H,W): softmax over the neighbours of mean_k -|x_k(p) - x_k(q_j)| / (1e-8 + 0.1 sigma_k),
    sigma_k the unbiased deviation of the 9 D samples (8 neighbours and the centre per dilation), from their mean."""
    x = images.to(dtype)
    D = len(dilations)
    nb = neighbours(x, dilations)                                                   # (B,K,8D,H,W)
    samples = torch.cat([nb, x[:, :, None].expand(-1, -1, D, -1, -1)], dim=2)       # (B,K,9D,H,W)
    mean = samples.mean(dim=2, keepdim=True)
    sigma = ((samples - mean) ** 2).sum(dim=2, keepdim=True).div(9 * D - 1).sqrt()
    a = (-(x[:, :, None] - nb).abs() / (1e-8 + 0.1 * sigma)).mean(dim=1)            # (B,P,H,W)
    return torch.softmax(a, dim=1)


def propagate(weights, scores, num_iter=10, dilations=DILATIONS):
    """scores (B,C,H,W) -> num_iter times m'_c(p) = sum_j w(p,j) m_c(q_j), in the dtype of ``weights``."""
    m = scores.to(weights.dtype)
    for _ in range(num_iter):
        m = (neighbours(m, dilations) * weights[:, None]).sum(dim=2)
    return m


def pamr(images, scores, num_iter=10, dilations=DILATIONS, dtype=torch.float64):
    return propagate(affinity(images, dilations, dtype), scores, num_iter, dilations)


def labels(scores, thresh=0.5, min_conf=0.0, ignore_index=255):
    """(B,C,H,W) -> int64 (B,H,W): C >= 2 the first maximum's index, ignore_index where the maximum is < min_conf;
    C == 1: scores >= thresh."""
    if scores.shape[1] == 1:
        return (scores[:, 0] >= thresh).long()
    best = scores.amax(dim=1)
    first = (scores == best[:, None]).float().argmax(dim=1)          # (argmax returns the FIRST maximal index)
    return torch.where(best < min_conf, torch.full_like(first, ignore_index), first)


def label_margin(scores, thresh=0.5, min_conf=0.0):
    """How far each pixel's decision is from flipping: the distance to thresh (C == 1); the smaller of the gap between the
    two largest channels and the distance of the largest to min_conf (C >= 2)."""
    if scores.shape[1] == 1:
        return (scores[:, 0] - thresh).abs()
    top = scores.topk(2, dim=1).values
    return torch.minimum(top[:, 0] - top[:, 1], (top[:, 0] - min_conf).abs())


# (B, H, W, C, K, dilations) of the device parity tests: 5 x 7 makes both borders clamp at once; 37 x 53 has odd rows, a tail
# in every direction and a batch stride; 64 x 64 another D and another C; 96 x 130 crosses a 64 x 4 workgroup tile both ways
CASES = ((1, 5, 7, 1, 1, DILATIONS), (2, 37, 53, 2, 3, DILATIONS), (2, 64, 64, 3, 3, (1, 3)), (1, 96, 130, 2, 3, DILATIONS))


def make_inputs(B, H, W, C, K, seed):
    """Images: conftest.smooth_image with a hard vertical edge (the right half 0.35 brighter); scores: uniform noise in
    [0, 0.5) with a block raised by 0.5, a different one per channel.  float32."""
    from conftest import smooth_image
    img = smooth_image(B, H, W, seed)[:, :K].clone()
    img[..., W // 2:] = (img[..., W // 2:] + 0.35).clamp(0, 1)
    g = torch.Generator().manual_seed(seed + 1000)
    m = 0.5 * torch.rand(B, C, H, W, generator=g)
    for c in range(C):
        y0, x0 = (H // 8) * (c % 3), (W // 8) * (c % 3)
        m[:, c, y0 + H // 4:y0 + 3 * H // 4, x0 + W // 4:x0 + 3 * W // 4] += 0.5
    return img.contiguous(), m.contiguous()
