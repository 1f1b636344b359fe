#!/usr/bin/env python3
"""Timing of the distance transforms (csrc/edt.hip) and what is built on them, at the two segmentation batch shapes,
labels (16,256,256) and (8,512,512).

Per shape and content, ``ops.edt`` for both planes, each metric:
  blobs        random discs of two classes (the shape of a pseudo mask)
  disc         one centred disc of radius H/4
  all-in       every pixel is IN, border=False: d2_out has no site at all.  The row pass sees a row without a site and writes
               the sentinel without walking; d2_in is all zero
  all-in+edge  every pixel is IN, border=True: the only sites of d2_out are outside the image
  corner       one IN pixel in a corner: the longest walks of the row pass (d2_in: up to W steps per pixel)
Algorithmic bytes: the labels read once (8 B/px) and the two planes written once (4 B/px each) = 16 B/px; the GB/s are
those bytes over the time, not memory rates (the column pass writes the planes once more and the row pass reads them back).
Comparisons, measured in the same run (no ratio is fixed in advance):
  biou         ops.boundary_iou_counts (two transforms of one plane each + the counts; ratio 0.02) against the same definition
               with torch ops on the device: ``width`` iterated 3 x 3 minimum pools on the padded masks and boolean sums
  scipy        ops.edt + the copy of both planes to the host against scipy.ndimage.distance_transform_edt of both polarities
               on the host + the copy of the labels to it (where scipy is importable; one round)
  criterion    wnn.BoundaryAwareCrossEntropyLoss forward + backward against wnn.CrossEntropyLoss with a pixel weight in
               place: the cost of the geometry
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds, min .. max beside the
mean.  Writes profiles/edt_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from weaklysuperviseddl_amd import ops, nn as wnn  # noqa: E402

SHAPES = ((16, 256, 256), (8, 512, 512))
BYTES_PER_PIXEL = 8 + 4 + 4


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def blobs(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        for k in range(6):
            cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            r = int(torch.randint(H // 16, H // 4, (1,), generator=g))
            out[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 2 if k == 5 else 1
    return out.to(dev)


def contents(B, H, W, dev):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = ((yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= (H // 4) ** 2).long()[None].repeat(B, 1, 1).to(dev)
    ones = torch.ones(B, H, W, dtype=torch.int64, device=dev)
    corner = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    corner[:, 0, 0] = 1
    return [("blobs", blobs(B, H, W, dev), False), ("disc", disc, False), ("all-in", ones, False), ("all-in+edge", ones, True),
            ("corner", corner, False)]


def torch_boundary_counts(preds, labels, width):
    """The published definition with the tensor library's kernels on the device: (B,2) int64."""
    def band(m):
        e = m[:, None].float()
        for _ in range(width):
            e = -F.max_pool2d(-F.pad(e, (1, 1, 1, 1), value=0.0), 3, stride=1)
        return m & ~(e[:, 0] > 0.5)
    a, b = band(preds == 1), band(labels == 1)
    return torch.stack([(a & b).flatten(1).sum(1), (a | b).flatten(1).sum(1)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edt_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    lines = [f"tools/edt_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, the "
             f"variants alternating inside a round; us = mean (min .. max over the rounds); GB/s = algorithmic bytes ({BYTES_PER_PIXEL} "
             "B/px: labels read once, two int32 planes written once) over the time"]
    for B, H, W in SHAPES:
        n = B * H * W
        variants = []
        for name, labels, border in contents(B, H, W, dev):
            for metric in ("euclid", "chebyshev"):
                bufs = {}
                variants.append((f"edt {name:12s} {metric:9s}", n * BYTES_PER_PIXEL,
                                 lambda labels=labels, metric=metric, border=border, bufs=bufs: ops.edt(labels, metric=metric, border=border, out=bufs)))
        gt = blobs(B, H, W, dev, 1)
        pred = torch.roll(gt, (3, -2), (1, 2)).contiguous()
        width = ops.boundary_width(H, W, 0.02)
        same = torch.equal(ops.boundary_iou_counts(pred, gt, width), torch_boundary_counts(pred, gt, width))
        i_biou = len(variants)
        variants.append((f"biou: ops.boundary_iou_counts, width {width}", 0, lambda: ops.boundary_iou_counts(pred, gt, width)))
        variants.append((f"biou: torch ops on the device ({width} min-pools per mask)", 0, lambda: torch_boundary_counts(pred, gt, width)))
        logits = torch.randn(B, 2, H, W, device=dev, requires_grad=True)
        masks = (gt == 1).long()
        aware = wnn.BoundaryAwareCrossEntropyLoss(sigma=3.0, floor=0.1)
        plain = wnn.CrossEntropyLoss().set_pixel_weight(ops.boundary_confidence(masks, 3.0, 0.1))

        def fwd_bwd(crit):
            logits.grad = None
            crit(logits, masks).backward()
        i_crit = len(variants)
        variants.append(("criterion: BoundaryAwareCrossEntropyLoss forward + backward", 0, lambda: fwd_bwd(aware)))
        variants.append(("criterion: CrossEntropyLoss with a pixel weight in place, forward + backward", 0, lambda: fwd_bwd(plain)))
        for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
            for _ in range(3):
                fn()
        rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
        lines.append(f"labels ({B},{H},{W}), {n} pixels, {n * BYTES_PER_PIXEL / 1e6:.1f} MB algorithmic; device counts == torch counts: {same}:")
        means = []
        for i, (name, nbytes, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            mean = sum(t) / len(t)
            means.append(mean)
            rate = f"{nbytes / mean / 1e3:8.1f} GB/s" if nbytes else ""
            lines.append(f"  {name:84s} {mean:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})  {rate}")
        worst = max(range(i_biou), key=lambda i: means[i])
        lines.append(f"  slowest content: {variants[worst][0].strip()} at {means[worst] / means[0]:.1f}x of blobs / euclid; the torch formulation of "
                     f"Boundary IoU takes {means[i_biou + 1] / means[i_biou]:.1f}x of ops.boundary_iou_counts; the geometry adds "
                     f"{means[i_crit] - means[i_crit + 1]:.1f} us to the criterion's forward + backward ({means[i_crit] / means[i_crit + 1]:.2f}x)")
        if ndi is not None:
            labels = contents(B, H, W, dev)[0][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_out, d_in = ops.edt(labels)
            host = (d_out.cpu(), d_in.cpu())
            t_dev = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            m = (labels.cpu() == 1).numpy()
            # (scipy would transform the batch as one volume: image by image)
            ref = [torch.stack([torch.from_numpy(ndi.distance_transform_edt(x) ** 2).round().long() for x in mm]) for mm in (m, ~m)]
            t_host = (time.perf_counter() - t0) * 1e6
            ok = torch.equal(host[0].long(), ref[0]) and torch.equal(host[1].long(), ref[1])
            lines.append(f"  scipy (blobs, one round, host clock): ops.edt + both planes to the host {t_dev:.0f} us; scipy.ndimage.distance_transform_edt "
                         f"of both polarities per image on the host {t_host:.0f} us ({t_host / t_dev:.0f}x); equal: {ok}")
        else:
            lines.append("  scipy: not importable here - not measured")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
