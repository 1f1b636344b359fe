"""Oracle of the distance transforms, boundary bands, Boundary IoU and boundary confidence (include/wsdl_hip.h "distance
transforms"), written from the contract by brute force in torch int64: per image the squared distance of every pixel to
every site, and the minimum.  Fine up to a few thousand pixels per image.

A pixel is IN where ``labels == value`` and OUT elsewhere.  ``d2_out`` = squared distance to the nearest OUT pixel, ``d2_in`` to
the nearest IN pixel; ``FAR`` where there is none.  ``border=True`` - everything outside the image is OUT for ``d2_out`` - is
implemented by padding: one ring of OUT pixels around the image (the nearest pixel outside an image is always in that
ring), the transform of the padded image, cropped.  ``band`` is defined WITHOUT distances, by the erosion the published
Boundary IoU (Cheng et al., CVPR 2021) uses."""
import torch
import torch.nn.functional as F

FAR = 1 << 30
METRICS = ("euclid", "chebyshev")


def _pair_d2(q, s, metric):
    """q (n,2), s (m,2) int64 coordinates -> (n,m) squared distances."""
    dy = (q[:, None, 0] - s[None, :, 0]).abs()
    dx = (q[:, None, 1] - s[None, :, 1]).abs()
    return dy * dy + dx * dx if metric == "euclid" else torch.maximum(dy, dx) ** 2


def _nearest(sites, metric, chunk=512):
    """sites bool (H,W) -> int64 (H,W): min over the sites of the squared distance, FAR without a site."""
    H, W = sites.shape
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    q = torch.stack([yy.flatten(), xx.flatten()], dim=1)
    s = q[sites.flatten()]
    if s.shape[0] == 0:
        return torch.full((H, W), FAR, dtype=torch.int64)
    out = torch.cat([_pair_d2(q[i:i + chunk], s, metric).min(dim=1).values for i in range(0, q.shape[0], chunk)])
    return out.view(H, W)


def dist2(labels, value=1, metric="euclid", border=False):
    """labels (B,H,W) integer or bool -> (d2_out, d2_in), int64 (B,H,W)."""
    assert metric in METRICS
    inside = labels.to(torch.int64) == int(value)
    d_out, d_in = [], []
    for m in inside:
        d_in.append(_nearest(m, metric))
        if border:
            d_out.append(_nearest(~F.pad(m, (1, 1, 1, 1), value=False), metric)[1:-1, 1:-1])
        else:
            d_out.append(_nearest(~m, metric))
    return torch.stack(d_out), torch.stack(d_in)


def erode(mask, width):
    """bool (B,H,W) -> ``width`` times a 3 x 3 minimum on the mask padded with background (zeros)."""
    m = mask.to(torch.float32)[:, None]
    for _ in range(int(width)):
        m = -F.max_pool2d(-F.pad(m, (1, 1, 1, 1), value=0.0), 3, stride=1)
    return m[:, 0] > 0.5


def band(mask, width):
    """The boundary region of Boundary IoU: the mask minus its ``width``-times eroded self."""
    mask = mask.to(torch.bool)
    return mask & ~erode(mask, width)


def boundary_iou_counts(preds, labels, width, value=1):
    """[(intersection, union)] per image of the two boundary regions, Python ints."""
    a, b = band(preds.to(torch.int64) == value, width), band(labels.to(torch.int64) == value, width)
    return [(int((x & y).sum()), int((x | y).sum())) for x, y in zip(a, b)]


def mean_iou(counts, EMPTY=1.0):
    """The mean over the images of intersection / union in Python floats, EMPTY for an empty union; summed in order."""
    per = [float(i) / float(u) if u else EMPTY for i, u in counts]
    acc = per[0]
    for v in per[1:]:
        acc += v
    return acc if len(per) == 1 else acc / len(per)


def boundary_width(H, W, ratio=0.02):
    return max(1, int(round(ratio * (H * H + W * W) ** 0.5)))


def boundary_iou(preds, labels, ratio=0.02, width=None, value=1):
    if width is None:
        width = boundary_width(labels.shape[1], labels.shape[2], ratio)
    return mean_iou(boundary_iou_counts(preds, labels, width, value))


def confidence(d2_out, d2_in, sigma=3.0, floor=0.0, dtype=torch.float64):
    """w = floor + (1 - floor) (1 - exp(-d2 / (2 sigma^2))), d2 = d2_out + d2_in; 1 where either plane holds FAR.  In ``dtype``."""
    d2 = (d2_out + d2_in).to(dtype)
    w = floor + (1 - floor) * (1 - torch.exp(-d2 / (2 * sigma ** 2)))
    return torch.where((d2_out >= FAR) | (d2_in >= FAR), torch.ones_like(w), w)


# (B, H, W) of the device tests: a single pixel, a single row, a single column; 5 x 7; 37 x 53 - odd sizes, a batch stride, two
# 32-column tiles and two 32-row words of the column pass; 64 x 64 - full words and tiles; 3 x 300 and 2 x 1100 - rows wider
# than one and than four 256-thread workgroups of the row pass; 300 x 3 - more 32-row words than a column workgroup holds at once
CASES = ((1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (3, 37, 53), (2, 64, 64), (1, 3, 300), (1, 2, 1100), (1, 300, 3))


def make_labels(B, H, W, seed):
    """int64 (B,H,W) in {0, 1, 2, 255}: discs of class 1 and 2, thin lines and isolated pixels of class 1, void patches.
    Images smaller than 64 pixels are drawn pixel by pixel."""
    g = torch.Generator().manual_seed(seed)
    if H * W < 64:
        return torch.tensor([0, 1, 1, 2, 255])[torch.randint(0, 5, (B, H, W), generator=g)].contiguous()

    def ri(lo, hi):
        return int(torch.randint(lo, max(hi, lo + 1), (1,), generator=g))

    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        for k in range(4):
            cy, cx, r = ri(0, H), ri(0, W), ri(1, max(2, min(max(H, 8), max(W, 8)) // 3))
            out[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 2 if k == 3 else 1
        y, x = ri(0, H), ri(0, W)
        out[b, y, ri(0, W // 2):ri(W // 2, W)] = 1                                  # a one-pixel row segment
        out[b, ri(0, H // 2):ri(H // 2, H), x] = 1                                  # a one-pixel column segment
        for _ in range(3):
            out[b, ri(0, H), ri(0, W)] = 1                                          # isolated pixels
        y0, x0 = ri(0, H), ri(0, W)
        out[b, y0:y0 + max(1, H // 6), x0:x0 + max(1, W // 6)] = 255                # a void patch
    return out.contiguous()
