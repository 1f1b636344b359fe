#!/usr/bin/env python3
"""Timing of the device-wide component labelling and seeded region growing (csrc/components_grid.hip) at scores
(16,2,256,256), (8,2,512,512) and (16,21,256,256).  No number is fixed in advance; everything below is measured in the same run,
the variants alternating inside a round.

  kernel       wsdl_label_components on the argmax map (three launches) and the whole wsdl_seeded_region_growing (six launches
               and a memset), straight through the C ABI
  criterion    wnn.SeededRegionGrowingLoss forward + backward from Python, beside wnn.CrossEntropyLoss on the same logits
  yardsticks   ops.keep_largest_batched on the foreground mask of the same argmax map (the one-workgroup-per-image labelling;
               it also picks the largest component, which the new call does not) and scipy.ndimage.label on the host, the
               copies to and from the device included
  content      random blobs (the argmax of smooth random logits), one component per image, and the serpentine - a one-pixel
               path through every other row, the longest parent chains across the tile seams: the expected worst case
Device-event times over back-to-back calls, three rounds, min .. max beside the mean; scipy by the host clock.  The first
section is the register and LDS use of every kernel (hipcc -Rpass-analysis=kernel-resource-usage; needs no GPU:
``--resources-only`` writes just that section and ``--resources-from FILE`` takes it from such a file instead of compiling).
Writes profiles/srg_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 2, 256, 256), (8, 2, 512, 512), (16, 21, 256, 256))


def kernel_name(mangled):
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    return name + {"Ix": "<int64>", "Ii": "<int32>"}.get(rest[:2], "")


def resource_lines():
    from weaklysuperviseddl_amd import _build
    src = os.path.join(_build.CSRC, "components_grid.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "o.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("srg_bench: hipcc failed:\n" + r.stderr[-2000:])
    lines = [f"register and LDS use of csrc/components_grid.hip ({' '.join(_build.FLAGS)} -Rpass-analysis=kernel-resource-usage):"]
    cur = None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: +Function Name: (.*?) \[-Rpass", ln)
        if m:
            cur = {"name": kernel_name(m.group(1))}
            continue
        m = re.search(r"remark: +(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                lines.append(f"  {cur['name']:30s} VGPRs {cur.get('VGPRs', -1):3d}  SGPRs {cur.get('TotalSGPRs', -1):3d}  scratch "
                             f"{cur.get('ScratchSize [bytes/lane]', -1):2d} B/lane  occupancy {cur.get('Occupancy [waves/SIMD]', -1)} waves/SIMD  "
                             f"LDS {cur['LDS Size [bytes/block]']} B")
                cur = None
    return lines


def time_round(torch, fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def serpentine(torch, B, H, W):
    m = torch.zeros(B, H, W, dtype=torch.int64)
    m[:, 0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[:, y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srg_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--resources-from", default=None)
    args = ap.parse_args()
    res = open(args.resources_from).read().splitlines() if args.resources_from else resource_lines()
    if args.resources_only:
        text = "\n".join(res) + "\n"
        print(text, end="")
        with open(args.out, "w") as f:
            f.write(text)
        return
    import numpy as np
    import torch
    import torch.nn.functional as F
    from scipy import ndimage
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd._lib import lib
    if not torch.cuda.is_available():
        raise SystemExit("srg_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    L = lib()
    eight = np.ones((3, 3), dtype=bool)
    lines = res + [f"tools/srg_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, "
                   "the variants alternating inside a round; us = mean (min .. max over the rounds)"]
    for B, Cc, H, W in SHAPES:
        g = torch.Generator().manual_seed(0)
        smooth = F.interpolate(torch.randn(B, Cc, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear", align_corners=False)
        logits = (3.0 * smooth + 0.05 * torch.randn(B, Cc, H, W, generator=g)).to(dev).requires_grad_()
        probs = torch.softmax(logits.detach(), dim=1).contiguous()
        arg = probs.argmax(dim=1)
        seeds = torch.where(torch.rand(B, H, W, generator=g).to(dev) < 0.02, arg, torch.full_like(arg, -100))
        contents = {"blobs": arg.contiguous(), "one component": torch.ones_like(arg), "serpentine": serpentine(torch, B, H, W).to(dev)}
        masks = {k: (v > 0).to(torch.uint8).contiguous() for k, v in contents.items()}
        comp = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        grown, counts = torch.empty(B, H, W, dtype=torch.int64, device=dev), torch.empty(B, Cc, dtype=torch.int64, device=dev)
        thresh = torch.tensor([0.7] + [0.55] * (Cc - 1)).to(dev)
        ws = ops.workspace(max(L.wsdl_label_components_workspace(B, H, W), L.wsdl_seeded_region_growing_workspace(B, Cc, H, W)), dev)
        stream = ops.raw_stream(dev)

        def k_label(lab):
            return lambda: ops.check(L.wsdl_label_components(lab.data_ptr(), B, H, W, 8, 0, 0, comp.data_ptr(), None, ws.data_ptr(),
                                                             ws.numel(), stream))

        def k_srg():
            ops.check(L.wsdl_seeded_region_growing(probs.data_ptr(), seeds.data_ptr(), None, thresh.data_ptr(), None, B, Cc, H, W, 255,
                                                   grown.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        srg, plain = wnn.SeededRegionGrowingLoss(thresh=(0.7, 0.55)).to(dev), wnn.CrossEntropyLoss()

        def fwd_bwd(crit, labels):
            logits.grad = None
            crit(logits, labels).backward()

        def host_label(lab):
            t0 = time.perf_counter()
            h = lab.cpu().numpy()
            out = np.stack([ndimage.label(h[b] > 0, structure=eight)[0] for b in range(B)])
            torch.from_numpy(out).to(dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6
        variants = [(f"kernel: wsdl_label_components, {k} (C ABI)", k_label(v)) for k, v in contents.items()]
        variants += [("kernel: wsdl_seeded_region_growing, blobs (C ABI, six launches + memset)", k_srg)]
        variants += [(f"yardstick: ops.keep_largest_batched, {k}", (lambda m: lambda: ops.keep_largest_batched(m))(m)) for k, m in masks.items()]
        variants += [("criterion: wnn.SeededRegionGrowingLoss forward + backward", lambda: fwd_bwd(srg, seeds)),
                     ("criterion: wnn.CrossEntropyLoss forward + backward", lambda: fwd_bwd(plain, arg))]
        for _name, fn in variants:              # warm up every variant: code objects load at the first launch
            for _ in range(3):
                fn()
        k_srg()
        labelled = int((grown != 255).sum())
        ncomp = int((ops.label_components(contents["blobs"]) == torch.arange(H * W, device=dev, dtype=torch.int32).view(1, H, W)).sum())
        rounds = [[time_round(torch, fn, args.reps) for _name, fn in variants] for _ in range(args.rounds)]
        host = {k: sorted(host_label(v) for _ in range(3))[1] for k, v in contents.items()}
        lines.append(f"scores ({B},{Cc},{H},{W}): {ncomp} components in the blobs' argmax map, {labelled} of {B * H * W} pixels labelled by the "
                     f"region growing from seeds on 2 % of them:")
        means = []
        for i, (name, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            means.append(sum(t) / len(t))
            lines.append(f"  {name:80s} {means[-1]:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})")
        for k, v in host.items():
            lines.append(f"  {'yardstick: scipy.ndimage.label on the host with both copies, ' + k:80s} {v:10.2f} us (median of 3)")
        lines.append(f"  label_components takes {means[0] / means[4]:.3f}x of keep_largest_batched on the blobs, {means[1] / means[5]:.3f}x on one "
                     f"component, {means[2] / means[6]:.3f}x on the serpentine, and {means[0] / host['blobs']:.4f}x of scipy with its copies; the "
                     f"serpentine - the longest chains across the seams - takes {means[2] / means[0]:.2f}x of the blobs, one component "
                     f"{means[1] / means[0]:.2f}x; the whole "
                     f"region growing takes {means[3] / means[0]:.2f}x of its labelling; wnn.SeededRegionGrowingLoss takes "
                     f"{means[7] / means[8]:.2f}x of wnn.CrossEntropyLoss (+{means[7] - means[8]:.1f} us)")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
