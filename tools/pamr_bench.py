#!/usr/bin/env python3
"""Timing of pixel-adaptive mask refinement (csrc/pamr.hip) at the two segmentation batch shapes, images (16,3,256,256) and
(8,3,512,512), scores with C = 2, the default dilations (1,2,4,8,12,24) and 10 iterations.

Per shape:
  weights     ops.pamr_affinity: one launch; reads the image (12 B/px), writes the 48 weight planes (192 B/px)
  iterations  ops.pamr(affinity=) with num_iter 10: ten launches; each reads the 48 planes (192 B/px) and reads and writes the
              two score channels (8 + 8 B/px; the neighbour gathers hit the same planes)
  pamr        ops.pamr: both
  labels      ops.pamr_labels (scores read, int64 written)
  torch       the same contract written with torch ops in float32 on the device: clamped index gathers into (B,K,9D,H,W) and
              (B,C,8D,H,W) tensors, torch.std, softmax, a weighted sum per iteration
and for context at the same shape (other refiners, other arithmetic - not the same result):
  ncut        refine_pseudo_masks_batched at the alternation's defaults (10 steps, six launches each; an alternation runs it 5 times)
  crf         ops.dense_crf at its defaults (two labels, 5 mean-field iterations)
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds, min .. max beside the mean.
No ratio is fixed in advance: the file records what was measured.  Writes profiles/pamr_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from weaklysuperviseddl_amd import ops  # noqa: E402

SHAPES = ((16, 3, 256, 256), (8, 3, 512, 512))
C_SCORES = 2
NUM_ITER = 10


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def smooth_images(B, K, H, W, dev):
    """Piece-wise smooth images in [0,1] with a hard vertical edge (the recipe of the tests, made on the device)."""
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    f = torch.rand(B, K, 4, 3, device=dev, generator=g) * torch.tensor([3.0, 3.0, 6.28], device=dev)
    img = (0.25 * torch.sin(6.28 * (f[..., 0, None, None] * yy + f[..., 1, None, None] * xx) + f[..., 2, None, None])).sum(2)
    img = img * 0.5 + 0.5 + 0.01 * torch.randn(B, K, H, W, device=dev, generator=g)
    img[..., W // 2:] += 0.35
    return img.clamp(0, 1).contiguous()


class TorchPamr:
    """The contract with the tensor library's own kernels, float32, on the device (index tensors made once)."""

    def __init__(self, H, W, dilations, dev):
        self.D = len(dilations)
        offs = [(dy * d, dx * d) for d in dilations for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
        self.iy = [(torch.arange(H, device=dev) + oy).clamp(0, H - 1) for oy, _ in offs]
        self.ix = [(torch.arange(W, device=dev) + ox).clamp(0, W - 1) for _, ox in offs]

    def neighbours(self, t):
        return torch.stack([t[..., iy, :][..., ix] for iy, ix in zip(self.iy, self.ix)], dim=2)

    def __call__(self, x, m, num_iter):
        nb = self.neighbours(x)
        samples = torch.cat([nb, x[:, :, None].expand(-1, -1, self.D, -1, -1)], dim=2)
        sigma = samples.std(dim=2, keepdim=True, unbiased=True)
        w = torch.softmax((-(x[:, :, None] - nb).abs() / (1e-8 + 0.1 * sigma)).mean(dim=1), dim=1)
        for _ in range(num_iter):
            m = (self.neighbours(m) * w[:, None]).sum(dim=2)
        return m


def variants_for(shape, dev):
    from weaklysuperviseddl_amd.TraditionalModel.AlternatingDirectionCutLoss import refine_pseudo_masks_batched
    B, K, H, W = shape
    dil = ops.PAMR_DILATIONS
    P = 8 * len(dil)
    x = smooth_images(B, K, H, W, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    m = 0.5 * torch.rand(B, C_SCORES, H, W, device=dev, generator=g)
    m[:, 1, H // 4:3 * H // 4, W // 4:3 * W // 4] += 0.5
    w = ops.pamr_affinity(x, dil)
    out = torch.empty_like(m)
    tp = TorchPamr(H, W, dil, dev)
    err = (tp(x, m, NUM_ITER) - ops.pamr(x, m, NUM_ITER, dil)).abs().max().item()
    # context: the two refiners the pipeline has
    S = torch.softmax(4 * (m - 0.5), dim=1).contiguous()
    masks = (m[:, 1] > 0.5).to(torch.uint8) * 255
    holder = torch.nn.Linear(1, 1).to(dev)            # (refine_pseudo_masks_batched takes the device from a model; S is given)
    cache = ops.pairwise_cache(x, 5, 0.1)
    cam = m[:, 1].contiguous()
    px_w, px_i = 4 * (K + P), 4 * (P + 2 * C_SCORES)
    variants = [
        ("weights: ops.pamr_affinity (1 launch)", px_w, lambda: ops.pamr_affinity(x, dil)),
        (f"iterations: ops.pamr(affinity=), {NUM_ITER} launches", NUM_ITER * px_i, lambda: ops.pamr(x, m, NUM_ITER, dil, affinity=w, out=out)),
        (f"pamr: ops.pamr, 1 + {NUM_ITER} launches", px_w + NUM_ITER * px_i, lambda: ops.pamr(x, m, NUM_ITER, dil, out=out)),
        ("labels: ops.pamr_labels", 4 * C_SCORES + 8, lambda: ops.pamr_labels(out)),
        ("torch: the same contract with torch ops, float32, on the device", 0, lambda: tp(x, m, NUM_ITER)),
        ("context ncut: refine_pseudo_masks_batched, 10 steps (x 5 per alternation)", 0,
         lambda: refine_pseudo_masks_batched(holder, x, masks, threshold=0.3, lr=1e-4, num_steps=10, lambda_boundary=0.1, S=S, affinity_cache=cache)),
        ("context crf: ops.dense_crf, defaults", 0, lambda: ops.dense_crf(x, cam)),
    ]
    return variants, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pamr_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pamr_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/pamr_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, the "
             "variants alternating inside a round; us = mean (min .. max over the rounds); B/px = algorithmic bytes per pixel (0: not "
             "counted - the tensor library's temporaries and the other refiners' traffic are their own)"]
    for shape in SHAPES:
        variants, err = variants_for(shape, dev)
        for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
            for _ in range(3):
                fn()
        rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
        n = shape[0] * shape[2] * shape[3]
        planes_mb = n * 4 * 8 * len(ops.PAMR_DILATIONS) / 1e6
        lines.append(f"images {shape}, scores C = {C_SCORES}, dilations {ops.PAMR_DILATIONS}, {n} pixels; weight planes {planes_mb:.0f} MB, written "
                     f"once and read {NUM_ITER} times = {planes_mb * (1 + NUM_ITER) / 1e3:.2f} GB; max |torch float32 - device| after {NUM_ITER} "
                     f"iterations {err:.1e}:")
        means = []
        for i, (name, bpp, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            mean = sum(t) / len(t)
            means.append(mean)
            rate = f"{bpp:5.0f} B/px {bpp * n / mean / 1e6:6.3f} TB/s" if bpp else " " * 23
            lines.append(f"  {name:76s} {mean:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})  {rate}")
        spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(len(variants)))
        lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  One iteration: {means[1] / NUM_ITER:.1f} us.  The torch "
                     f"formulation takes {means[4] / means[2]:.1f}x of ops.pamr; an alternation's ncut refinement (5 x the line above) "
                     f"{5 * means[5] / means[2]:.1f}x, the dense CRF {means[6] / means[2]:.1f}x.")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The planes are reused call after call and fit the last-level cache at the smaller "
                 "shape: the TB/s are algorithmic bytes over time, not HBM rates.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
