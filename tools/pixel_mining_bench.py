#!/usr/bin/env python3
"""Timing of pixel mining (csrc/pixel_mining.hip) at the two segmentation batch shapes, (16,2,256,256) and (8,2,512,512),
on random logits and on the worst case for the digit histograms (every pixel the same logits and label: every loss equal).

Per shape and input: the entry points the mined loss adds - wsdl_mining_valid (1 launch), wsdl_kth_value (memset + 4 histogram
passes + 1 result launch) and wsdl_mining_weights (2 launches) - then loss + gradient of
  mined      ops.cross_entropy_mined, hard (thresh 0.7, min_kept 100 000) and trim (drop_frac 0.25), batch and image scope
  floor      ops.cross_entropy with a pixel weight on the same build: what mining adds to
  torch      the tensor library's formulation on the device: F.cross_entropy(reduction='none'), topk, a mask, a weighted mean
             - with k FIXED on the host beforehand, i.e. WITHOUT the host read of the valid-pixel count that a real step
             needs every iteration (the stall is left out of torch's side, not of ours)
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds, min .. max beside the
mean, and the algorithmic bytes per pixel beside each line.  No ratio is fixed in advance: the file records what was measured.
Writes profiles/pixel_mining_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from weaklysuperviseddl_amd import ops  # noqa: E402

SHAPES = ((16, 2, 256, 256), (8, 2, 512, 512))


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def variants_for(shape, kind, dev):
    B, C, H, W = shape
    n = B * H * W
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "random":
        z = torch.randn(B, C, H, W, device=dev, generator=g) * 3.0
        y = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        y[torch.rand(B, H, W, device=dev, generator=g) < 0.2] = -100
    else:
        z = torch.zeros(B, C, H, W, device=dev)
        z[:, 1] = 0.5
        y = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    pw = torch.rand(B, H, W, device=dev, generator=g) + 0.05
    zg = z.clone().requires_grad_(True)
    one = torch.ones((), device=dev)
    lib, P, S = ops.lib(), ops._p, ops._stream
    nll = ops.cross_entropy(z, y, reduction="none")
    valid = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    tau, cnt = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    m, kept = torch.empty(B, H, W, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    ws = ops.workspace(max(lib.wsdl_kth_workspace(B), lib.wsdl_mining_weights_workspace(B)), dev)
    C2 = 4 * C            # logits read / gradient written, bytes per pixel

    def kth(segments, k, frac):
        return lambda: ops.check(lib.wsdl_kth_value(P(nll), P(valid), n // segments, segments, 1, k, frac, P(tau), P(cnt), P(ws), ws.numel(), S()))

    def weights(segments, mode):
        return lambda: ops.check(lib.wsdl_mining_weights(P(nll), P(valid), None, P(tau), 0.3567, mode, n // segments, segments, P(m), P(kept),
                                                         P(ws), ws.numel(), S()))

    def mined_fn(mode, **kw):
        def run():
            zg.grad = None
            ops.cross_entropy_mined(zg, y, mode=mode, **kw).backward(one)
        return run

    def floor():
        zg.grad = None
        ops.cross_entropy(zg, y, pixel_weight=pw).backward(one)

    k_fixed = max(1, int(0.25 * n))     # torch's side: k known beforehand (a real step reads the valid count from the device)

    def torch_topk():
        zg.grad = None
        l = F.cross_entropy(zg, y, reduction="none")
        thr = torch.topk(l.detach().flatten(), k_fixed, sorted=False).values.min()
        keep = ((l.detach() >= thr) & (y != -100)).float()
        ((l * keep).sum() / keep.sum()).backward()

    def torch_none():
        zg.grad = None
        F.cross_entropy(zg, y, reduction="none").sum().backward()

    # bytes per pixel: labels 8, a float map 4, the byte map 1
    out = [
        ("wsdl_mining_valid (labels -> byte map)", 8 + 1, lambda: ops.check(lib.wsdl_mining_valid(P(y), -100, None, P(valid), n, S()))),
        ("wsdl_kth_value, 1 segment (4 passes over nll + valid)", 4 * (4 + 1), kth(1, 100000, 0.0)),
        (f"wsdl_kth_value, {B} segments, k = 1 + 0.25 n", 4 * (4 + 1), kth(B, 1, 0.25)),
        ("wsdl_mining_weights, 1 segment", 4 + 1 + 4, weights(1, 0)),
        (f"wsdl_mining_weights, {B} segments", 4 + 1 + 4, weights(B, 1)),
        ("floor: ops.cross_entropy(pixel_weight=) loss + gradient", 2 * C2 + 8 + 4 + C2 * 2, floor),
        ("mined hard, thresh 0.7, min_kept 100000/B, batch", 0, mined_fn("hard", thresh=0.7, min_kept=100000 // B)),
        ("mined hard, thresh 0.7, min_kept 100000/B, image", 0, mined_fn("hard", thresh=0.7, min_kept=100000 // B, scope="image")),
        ("mined trim, drop_frac 0.25, batch", 0, mined_fn("trim", drop_frac=0.25)),
        ("mined trim, drop_frac 0.25, image", 0, mined_fn("trim", drop_frac=0.25, scope="image")),
        ("torch: CE(reduction='none') + sum, loss + gradient", 0, torch_none),
        ("torch: CE('none') + topk(fixed k) + masked mean, loss + gradient", 0, torch_topk),
    ]
    # the mined loss: the nll map (logits + labels read, map written), valid, select, weights, then the floor's traffic
    extra = (C2 + 8 + 4) + (8 + 1) + 4 * (4 + 1) + (4 + 1 + 4)
    floor_bytes = out[5][1]
    return [(name, (floor_bytes + extra) if name.startswith("mined") else b, fn) for name, b, fn in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_mining_bench.txt"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_mining_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/pixel_mining_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, "
             "the variants alternating inside a round; us = mean (min .. max over the rounds); B/px = algorithmic bytes per pixel "
             "(0: not counted - the tensor library's temporaries are its own)"]
    for shape in SHAPES:
        for kind in ("random", "all-equal"):
            variants = variants_for(shape, kind, dev)
            for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
                for _ in range(5):
                    fn()
            rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
            n = shape[0] * shape[2] * shape[3]
            lines.append(f"{shape}, {kind} logits, {n} pixels:")
            means = []
            for i, (name, bpp, _fn) in enumerate(variants):
                t = [r[i] for r in rounds]
                mean = sum(t) / len(t)
                means.append(mean)
                rate = f"{bpp:5.0f} B/px {bpp * n / mean / 1e6:6.3f} TB/s" if bpp else " " * 23
                lines.append(f"  {name:66s} {mean:9.2f} us ({min(t):9.2f} .. {max(t):9.2f})  {rate}")
            spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(len(variants)))
            lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  Mining adds {min(means[6:10]) - means[5]:.1f} .. "
                         f"{max(means[6:10]) - means[5]:.1f} us to the floor's {means[5]:.1f} us; the torch formulation without its host read of k "
                         f"takes {means[11]:.1f} us ({means[11] / max(means[6:10]):.2f}x .. {means[11] / min(means[6:10]):.2f}x of the mined loss).")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and, for the loss + "
                 "gradient lines, the host time of the call where the device waits for it.  The maps are reused call after call, so "
                 "the small ones are partly served by the last-level cache: the TB/s are not HBM rates.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
