#!/usr/bin/env python3
"""Timing of the multi-scale + flip fusion (csrc/multiscale.hip) at the shapes its callers produce:

  cam   LayerCAMGenerator.generate_multiscale at (16,1,224,224): four scales with mirror images, every source already at the
        target's size (16 x 2 images each), activation none, mean; then ops.max_normalize with the mask
  seg2  predict_multiscale at the target (16,2,256,256): the stride-8 head logits of six scales with mirror images, softmax, mean
  seg21 the same at (8,21,512,512)
Per shape: the fusion with scores + labels, labels only (no score planes), the same contract written with torch ops on the
device (interpolate, flip, softmax, add, argmax), and a plain device copy of the output tensor - the floor of a store-bound launch.
scale_flip is timed against ops.bilinear_resize + flip + cat at the two image shapes of the segmentation batches.
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds, min .. max beside the mean.
No ratio is fixed in advance: the file records what was measured.  Registers, LDS and scratch of every kernel come from the
compiler's resource remarks (``--resources FILE``: a saved copy of them; default: hipcc is asked again, which needs no device).
Writes profiles/multiscale_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from weaklysuperviseddl_amd import ops, _build  # noqa: E402

SEG_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def kernel_resources(saved=None):
    """[(kernel, VGPRs, SGPR spills, scratch bytes / lane, LDS bytes / block, waves / SIMD)] of csrc/multiscale.hip."""
    if saved:
        text = open(saved).read()
    else:
        src = os.path.join(_build.CSRC, "multiscale.hip")
        cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    out = []
    for r in rows:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", r["name"])            # (anonymous namespace)::<length><name>[I Li<N> E]...
        name = r["name"]
        if m:
            rest = name[m.end():]
            base, tail = rest[:int(m.group(1))], rest[int(m.group(1)):]
            t = re.match(r"ILi(\d+)E", tail)
            name = base + (f"<{t.group(1)}>" if t else "")
        out.append((name, r.get("VGPRs"), r.get("SGPRs Spill"), r.get("ScratchSize [bytes/lane]"), r.get("LDS Size [bytes/block]"),
                    r.get("Occupancy [waves/SIMD]")))
    return out


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def torch_fuse(srcs, size, B, act):
    acc = None
    for t in srcs:
        r = F.interpolate(t, size=size, mode="bilinear", align_corners=False) if tuple(t.shape[-2:]) != tuple(size) else t
        for part in (r[:B], r[B:].flip(-1)):
            if act == "softmax":
                part = part.softmax(dim=1)
            acc = part if acc is None else acc + part
    return acc / (2 * len(srcs))


def fusion_variants(name, B, C, H, W, sizes, act, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    srcs = [torch.randn(2 * B, C, h, w, device=dev, generator=g) * 2 for h, w in sizes]
    out = {}
    scores = ops.multiscale_fuse(srcs, (H, W), mirrored=True, activation=act)
    err = (scores - torch_fuse(srcs, (H, W), B, act)).abs().max().item()
    other, dst = torch.empty_like(scores), torch.empty_like(scores)
    lab_kw = dict(thresh=0.5)
    variants = [
        (f"{name}: ops.multiscale_fuse, scores + labels (1 launch)", lambda: ops.multiscale_fuse(srcs, (H, W), mirrored=True, activation=act, labels=True, out=out, **lab_kw)),
        (f"{name}: ops.multiscale_fuse, labels only (1 launch)", lambda: ops.multiscale_fuse(srcs, (H, W), mirrored=True, activation=act, scores=False, labels=True, out=out, **lab_kw)),
        (f"{name}: torch interpolate + flip + {act} + add" + (" + argmax" if C > 1 else " + threshold"),
         (lambda: torch_fuse(srcs, (H, W), B, act).argmax(dim=1)) if C > 1 else (lambda: torch_fuse(srcs, (H, W), B, act) >= 0.5)),
        (f"{name}: device copy of the scores tensor (store floor)", lambda: dst.copy_(other)),
    ]
    if C == 1:
        variants.insert(2, (f"{name}: ops.max_normalize with mask (memset + 2 launches)", lambda: ops.max_normalize(scores, 0.3, out=other)))
    return variants, err, scores.numel() * 4


def scale_flip_variants(shape, size, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(*shape, device=dev, generator=g)
    out = torch.empty(2 * shape[0], shape[1], *size, device=dev)

    def by_ops():
        r = ops.bilinear_resize(x, size)
        return torch.cat([r, r.flip(-1)])
    assert torch.equal(ops.scale_flip(x, size, True), by_ops())
    return [(f"scale_flip {shape} -> {size}: ops.scale_flip (1 launch)", lambda: ops.scale_flip(x, size, True, out=out)),
            (f"scale_flip {shape} -> {size}: ops.bilinear_resize + flip + cat", by_ops)], out.numel() * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiscale_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiscale_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/multiscale_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, the "
             "variants alternating inside a round; us = mean (min .. max over the rounds)"]

    def measure(variants, out_bytes, head):
        for _n, fn in variants:
            for _ in range(3):
                fn()
        rounds = [[time_round(fn, args.reps) for _n, fn in variants] for _ in range(args.rounds)]
        lines.append(head)
        means = []
        for i, (n, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            means.append(sum(t) / len(t))
            lines.append(f"  {n:92s} {means[-1]:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})")
        return means

    seg_hw = lambda H, W: [(h // 8, w // 8) for h, w in ops.multiscale_sizes(H, W, SEG_SCALES)]      # noqa: E731
    for name, B, C, H, W, sizes, act in (("cam", 16, 1, 224, 224, [(224, 224)] * 4, "none"),
                                         ("seg2", 16, 2, 256, 256, seg_hw(256, 256), "softmax"),
                                         ("seg21", 8, 21, 512, 512, seg_hw(512, 512), "softmax")):
        variants, err, nbytes = fusion_variants(name, B, C, H, W, sizes, act, dev)
        means = measure(variants, nbytes, f"target ({B},{C},{H},{W}) from {len(sizes)} sources {sizes} with mirrored halves, activation {act}, mean; "
                        f"scores {nbytes / 1e6:.1f} MB; max |torch float32 - device| {err:.1e}:")
        it, ic = len(variants) - 2, len(variants) - 1
        lines.append(f"  the fusion takes {means[0] / means[ic]:.2f}x of the copy of its output and {means[0] / means[it]:.3f}x of the torch formulation "
                     f"(labels only: {means[1] / means[it]:.3f}x)")
    for shape, size in (((16, 3, 256, 256), (384, 384)), ((8, 3, 512, 512), (768, 768))):
        variants, nbytes = scale_flip_variants(shape, size, dev)
        means = measure(variants, nbytes, f"scale_flip, output {nbytes / 1e6:.1f} MB:")
        lines.append(f"  ops.scale_flip takes {means[0] / means[1]:.3f}x of resize + flip + cat")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  A softmax fusion evaluates one expf per member, channel and output pixel (12 x C per "
                 "pixel here): those shapes are bound by the vector ALU, not by their stores - the ratio to the copy says by how much.")
    lines.append("kernel resources (compiler remarks, gfx950): kernel, VGPRs, SGPR spills, scratch B/lane, LDS B/block, waves/SIMD")
    for row in kernel_resources(args.resources):
        lines.append("  " + "  ".join(str(v) for v in row))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
