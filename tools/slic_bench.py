#!/usr/bin/env python3
"""Timing of the integer SLIC superpixels and of the pooling over them (csrc/slic.hip) at images (16,3,256,256) and
(8,3,512,512), step 8, 16 and 32, on smooth blobs, uniform noise and a flat image.  No number is fixed in advance - no GPU
baseline for SLIC exists here; everything below is measured in the same run, the variants alternating inside a round.

  whole call   wsdl_slic with num_iter = 10 straight through the C ABI, and the same launches replayed from a launch plan
               (plan.record(ops.slic, ...).replay(): one host call for all of them - what is left is the device's time)
  stages       the C ABI has one entry point, so the stages come from calls that differ by one stage: an iteration (assign +
               update) = (t[num_iter = 10] - t[num_iter = 1]) / 9; init + connectivity = t[num_iter = 1] minus one iteration; the
               labelling inside the connectivity pass = wsdl_label_components (4-connected, with areas) on the same raw map
  assignment   the bytes an iteration must move (3 bytes of image per pixel; the centres are re-read from LDS) over the time
               of an iteration, beside the rates MI355X_MICROARCH.md gives for the levels the working set lives in
  pooling      wsdl_superpixel_mean with the gather (superpixel_snap) at C = 2 and 21 on the blobs' segments
  yardstick    the numpy + scipy oracle (tests/slic_oracle.py) on the host, with the copies from and to the device
  context      refine_dataset(method="superpixel")'s device work on one chunk (quantise, slic, snap of a two-channel
               prediction) beside ops.pamr on the same chunk
Device-event times over back-to-back calls, three rounds, min .. max beside the mean; the oracle by the host clock.  The first
section is the register and LDS use of every kernel (hipcc -Rpass-analysis=kernel-resource-usage; needs no GPU:
``--resources-only`` writes just that section and ``--resources-from FILE`` takes it from such a file instead of compiling).
Writes profiles/slic_bench.txt (``--out`` elsewhere); ``--append FILE`` adds the lines of FILE (the bench.py comparison)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ((16, 256, 256), (8, 512, 512))
STEPS = (8, 16, 32)
CONTENTS = ("blobs", "noise", "flat")


def resource_lines():
    import re
    from srg_bench import kernel_name
    from weaklysuperviseddl_amd import _build
    src = os.path.join(_build.CSRC, "slic.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "o.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("slic_bench: hipcc failed:\n" + r.stderr[-2000:])
    lines = [f"register and LDS use of csrc/slic.hip ({' '.join(_build.FLAGS)} -Rpass-analysis=kernel-resource-usage):"]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slic_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--resources-from", default=None)
    ap.add_argument("--append", default=None)
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
    import slic_oracle as so
    from srg_bench import time_round
    from weaklysuperviseddl_amd import ops, plan
    from weaklysuperviseddl_amd._lib import lib
    if not torch.cuda.is_available():
        raise SystemExit("slic_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    L = lib()
    stream = ops.raw_stream(dev)
    lines = res + [f"tools/slic_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} rounds, "
                   "the variants alternating inside a round; us = mean (min .. max over the rounds); compactness 10"]

    def fmt(t):
        return f"{sum(t) / len(t):10.2f} us ({min(t):10.2f} .. {max(t):10.2f})"

    merge_share = {}
    for B, H, W in SHAPES:
        images = {c: torch.from_numpy(so.make_batch(c, B, H, W, seed=3)).to(dev) for c in CONTENTS}
        for step in STEPS:
            GH, GW = ops.slic_grid(H, W, step)
            n_max = ops.slic_max_segments(H, W, step)
            raw = torch.empty(B, H, W, dtype=torch.int32, device=dev)
            seg = torch.empty_like(raw)
            comp, area = torch.empty_like(raw), torch.empty_like(raw)
            cen = torch.empty(B, GH * GW, 5, dtype=torch.int32, device=dev)
            nseg = torch.empty(B, dtype=torch.int32, device=dev)
            ws = ops.workspace(max(L.wsdl_slic_workspace(B, H, W, step), L.wsdl_superpixel_workspace(B, 21, n_max)), dev)

            def k_slic(img, it):
                return lambda: ops.check(L.wsdl_slic(img.data_ptr(), B, H, W, step, 10, it, max(1, step * step // 4), raw.data_ptr(),
                                                     cen.data_ptr(), seg.data_ptr(), nseg.data_ptr(), ws.data_ptr(), ws.numel(), stream))
            raws = {}
            for c in CONTENTS:
                k_slic(images[c], 10)()
                raws[c] = raw.to(torch.int64)

            def k_label(lab):
                return lambda: ops.check(L.wsdl_label_components(lab.data_ptr(), B, H, W, 4, 0, 0, comp.data_ptr(), area.data_ptr(),
                                                                 ws.data_ptr(), ws.numel(), stream))
            variants, plans = [], []
            for c in CONTENTS:
                plans.append(plan.record(ops.slic, images[c], step, out={})[0])
                variants += [(c, 10, k_slic(images[c], 10)), (c, 1, k_slic(images[c], 1)), (c, "label", k_label(raws[c])),
                             (c, "plan", plans[-1].replay)]
            for _n, _i, fn in variants:
                for _ in range(3):
                    fn()
            rounds = [[time_round(torch, fn, args.reps) for _n, _i, fn in variants] for _ in range(args.rounds)]
            lines.append(f"images ({B},3,{H},{W}), step {step}: K = {GH * GW} centres per image, at most {n_max} segments")
            for j, c in enumerate(CONTENTS):
                t10, t1, tl, tp = ([r[4 * j + k] for r in rounds] for k in range(4))
                it = [(a - b) / 9 for a, b in zip(t10, t1)]
                conn = [b - i for b, i in zip(t1, it)]
                k_slic(images[c], 10)()
                torch.cuda.synchronize()
                n_b = nseg.cpu().numpy()
                mean10 = sum(t10) / len(t10)
                oracle = None
                if step == 16:                  # the host oracle takes seconds per image: once per shape and content
                    stats = {}
                    t0 = time.perf_counter()
                    host = images[c].cpu().numpy()
                    want = so.slic(host, step, stats=stats)
                    torch.from_numpy(want["segments"]).to(dev)
                    torch.cuda.synchronize()
                    t_host = (time.perf_counter() - t0) * 1e6
                    equal = np.array_equal(seg.cpu().numpy(), want["segments"]) and np.array_equal(n_b, want["n_segments"])
                    oracle = (f"{t_host:12.2f} us (once): the device call takes {mean10 / t_host:.5f}x; results equal: {equal}; "
                              f"{stats['orphans']} orphans of {stats['components']} components, longest chain {stats['chain']}")
                gbs = 3.0 * B * H * W / (sum(it) / len(it) * 1e-6) / 1e9
                merge_share[(B, H, W, step, c)] = (sum(conn) / len(conn), mean10)
                lines.append(f"  {c:6s} whole call, num_iter 10 (C ABI, {ops.slic_launches(H, W, 10)} launches)      {fmt(t10)}")
                lines.append(f"  {c:6s} the same launches replayed from a launch plan             {fmt(tp)}")
                lines.append(f"  {c:6s}   one iteration (assign + update)                  {fmt(it)}   {gbs:8.1f} GB/s of image bytes")
                lines.append(f"  {c:6s}   init + connectivity pass                         {fmt(conn)}")
                lines.append(f"  {c:6s}   of which labelling (wsdl_label_components, areas) {fmt(tl)}")
                lines.append(f"  {c:6s}   segments per image {int(n_b.min())} .. {int(n_b.max())}")
                if oracle:
                    lines.append(f"  {c:6s}   numpy oracle on the host with both copies       {oracle}")
            # pooling on the blobs' segments
            k_slic(images["blobs"], 10)()
            for Cc in (2, 21):
                vals = torch.randn(B, Cc, H, W, device=dev)
                mean = torch.empty(B, Cc, n_max, device=dev)
                cnt = torch.empty(B, n_max, dtype=torch.int32, device=dev)
                snapped = torch.empty_like(vals)

                def k_snap():
                    ops.check(L.wsdl_superpixel_mean(vals.data_ptr(), seg.data_ptr(), B, Cc, H, W, n_max, mean.data_ptr(), cnt.data_ptr(),
                                                     snapped.data_ptr(), ws.data_ptr(), ws.numel(), stream))
                for _ in range(3):
                    k_snap()
                t = [time_round(torch, k_snap, args.reps) for _ in range(args.rounds)]
                nbytes = 2.0 * 4 * B * Cc * H * W
                lines.append(f"  superpixel_snap, C = {Cc:2d}, blobs' segments (C ABI, 3 launches + 2 memsets) {fmt(t)}   "
                             f"{nbytes / (sum(t) / len(t) * 1e-6) / 1e9:8.1f} GB/s of values read + written")
    worst = max(merge_share, key=lambda k: merge_share[k][0])
    noise_worst = all(merge_share[(B, H, W, s, "noise")][0] >= max(merge_share[(B, H, W, s, c)][0] for c in CONTENTS) - 1e-9
                      for B, H, W in SHAPES for s in STEPS)
    lines.append(f"Noise was expected to be the worst case of the merge (nearly every component an orphan, the longest chains): the "
                 f"init + connectivity time is largest on noise at every shape and step: {noise_worst}; the largest one is "
                 f"{merge_share[worst][0]:.1f} us of a {merge_share[worst][1]:.1f} us call at {worst}.")
    lines.append("Assignment kernel against the memory system: an iteration must read 3 bytes per pixel (3.1 MB at 16x256x256, 6.3 MB at "
                 "8x512x512; every XCD reads its own tiles again each iteration, 0.4 - 0.8 MB: resident in its 4 MiB L2, 34.5 TB/s "
                 "aggregate per MI355X_MICROARCH.md; from the Infinity Cache 8.6 TB/s gathered, from HBM 6.3 TB/s) - the GB/s column above "
                 "is far below each.  The replayed plan takes the time of the call from the host, so the call is bound by the device, not "
                 "by the host's launches; the assignment kernel is bound by its arithmetic - nine 64-bit distance evaluations and two "
                 "packed 64-bit LDS atomics per pixel - not by memory.")

    # context: the device work of refine_dataset(method="superpixel") on one chunk beside ops.pamr on the same chunk
    B, H, W = 64, 256, 256
    g = torch.Generator().manual_seed(1)
    imgs = torch.nn.functional.interpolate(torch.randn(B, 3, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear").to(dev)
    S = torch.softmax(torch.randn(B, 2, H, W, generator=g).to(dev), dim=1).contiguous()
    n_max = ops.slic_max_segments(H, W, 16)

    def chunk_sp():
        segs, _ = ops.slic(ops.slic_quantize(imgs), 16)
        return ops.superpixel_snap(S, segs, n_max)[:, 1] > 0.3

    def chunk_pamr():
        return ops.pamr(imgs, S)[:, 1] > 0.3
    for fn in (chunk_sp, chunk_pamr):
        for _ in range(2):
            fn()
    t_sp = [time_round(torch, chunk_sp, 5) for _ in range(args.rounds)]
    t_pm = [time_round(torch, chunk_pamr, 5) for _ in range(args.rounds)]
    lines.append(f"context, one refine_dataset chunk of ({B},3,{H},{W}) without the network: method=\"superpixel\" (quantise, slic step 16, "
                 f"snap of 2 channels, threshold; from Python) {fmt(t_sp)}; method=\"pamr\" (ops.pamr defaults, threshold) {fmt(t_pm)}")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.")
    if args.append and os.path.exists(args.append):
        lines += open(args.append).read().splitlines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
