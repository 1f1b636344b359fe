#!/usr/bin/env python3
"""Timing of the overlap (soft Dice / Tversky) and focal losses (csrc/overlap_loss.hip) at the two segmentation batch shapes,
logits (16,2,256,256) and (8,2,512,512), all C = 2 classes listed.  No ratio is fixed in advance; everything below is measured
in the same run, the variants alternating inside a round.

  kernel       wsdl_tversky_fwd_bwd (three launches: sums, finalize, gradient) and wsdl_focal_fwd_bwd (two: fused pass, finalize)
               against wsdl_softmax_ce_ex_fwd_bwd with a pixel weight in place, all called straight through the C ABI.
               Algorithmic bytes per pixel: Tversky 2 x (4C logits + 8 labels) + 4C dlogits (the logits are read twice: the
               coefficients of the gradient need the sums of the whole segment first); focal 4C + 8 + 4C; cross entropy 4C +
               8 + 4 (pixel weight) + 4C.  The byte ratios stand next to the time ratios.  Both new kernels evaluate their
               softmax in double.
  criterion    wnn.DiceLoss, wnn.FocalLoss and wnn.CrossEntropyTverskyLoss forward + backward from Python, beside
               wnn.CrossEntropyLoss
  torch        the same contracts written with the tensor library's kernels on the device, forward + backward: soft Dice as
               one-hot, softmax, three sums and a mean; the focal loss as log_softmax, gather, exp, pow and a mean
Device-event times over back-to-back calls, three rounds, min .. max beside the mean.  The first section of the output is the
register use of every kernel instantiation (hipcc -Rpass-analysis=kernel-resource-usage on csrc/overlap_loss.hip; needs no
GPU: ``--resources-only`` writes just that section - of ``--resources-source`` another file of csrc/, e.g. boundary_loss.hip -
and ``--resources-from FILE`` takes it from such a file instead of compiling).
Writes profiles/overlap_loss_bench.txt (``--out`` elsewhere)."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 2, 256, 256), (8, 2, 512, 512))


def kernel_name(mangled):
    """``name<NC, V>`` from the Itanium name of a kernel in the anonymous namespace (the mangled name when it is none)."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    t = re.match(r"I((?:Li\d+E)+)E", rest)
    return name + ("<" + ", ".join(re.findall(r"Li(\d+)E", t.group(1))) + ">" if t else "")


def resource_lines(source="overlap_loss.hip"):
    """One line per kernel instantiation of csrc/<source> (or of the file at an absolute path): VGPRs, AGPRs, SGPRs, scratch,
    occupancy, LDS."""
    from weaklysuperviseddl_amd import _build
    src = os.path.join(_build.CSRC, source)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "o.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"overlap_loss_bench: hipcc failed for {source}:\n" + r.stderr[-2000:])
    text = r.stderr
    lines = [f"register use of csrc/{os.path.basename(source)} ({' '.join(_build.FLAGS)} -Rpass-analysis=kernel-resource-usage):"]
    cur, spills = None, 0
    for ln in text.splitlines():
        m = re.search(r"remark: +Function Name: (.*?) \[-Rpass", ln)
        if m:
            cur = {"name": kernel_name(m.group(1))}
            continue
        m = re.search(r"remark: +(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                spills += cur.get("ScratchSize [bytes/lane]", 0) > 0
                lines.append(f"  {cur['name']:40s} VGPRs {cur.get('VGPRs', -1):4d}  AGPRs {cur.get('AGPRs', -1):3d}  SGPRs {cur.get('TotalSGPRs', -1):4d}  "
                             f"scratch {cur.get('ScratchSize [bytes/lane]', -1):3d} B/lane  occupancy {cur.get('Occupancy [waves/SIMD]', -1)} waves/SIMD  "
                             f"LDS {cur['LDS Size [bytes/block]']} B")
                cur = None
    lines.append(f"  instantiations with scratch: {spills} (template arguments: <NC, V> - NC = C held in registers, 0 = any C with up to 32 "
                 "listed classes accumulated per lane; V = pixels per item)")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_loss_bench.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--resources-from", default=None)
    ap.add_argument("--resources-source", default="overlap_loss.hip", help="the file of csrc/ the register table is made of")
    args = ap.parse_args()
    if args.resources_from:
        res = open(args.resources_from).read().splitlines()
    else:
        res = resource_lines(args.resources_source)
    if args.resources_only:
        text = "\n".join(res) + "\n"
        print(text, end="")
        with open(args.out, "w") as f:
            f.write(text)
        return
    import torch
    import torch.nn.functional as F
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd._lib import lib
    if not torch.cuda.is_available():
        raise SystemExit("overlap_loss_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    L = lib()
    lines = res + [f"tools/overlap_loss_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} "
                   "rounds, the variants alternating inside a round; us = mean (min .. max over the rounds); GB/s = algorithmic bytes over the time"]
    for B, Cc, H, W in SHAPES:
        n = B * H * W
        g = torch.Generator().manual_seed(0)
        masks = torch.randint(0, Cc, (B, H, W), generator=g).to(dev)
        logits = torch.randn(B, Cc, H, W, generator=g).to(dev).requires_grad_()
        pw = torch.rand(B, H, W, generator=g).to(dev)
        raw = logits.detach()
        dl, loss, inv = torch.empty_like(raw), torch.empty((), device=dev), torch.empty(1, device=dev)
        ws = ops.workspace(max(L.wsdl_reduce_workspace(), L.wsdl_overlap_workspace(1, Cc)), dev)
        cls = (C.c_int * Cc)(*range(Cc))
        stream = ops.raw_stream(dev)

        def k_tversky():
            ops.check(L.wsdl_tversky_fwd_bwd(raw.data_ptr(), masks.data_ptr(), cls, Cc, loss.data_ptr(), dl.data_ptr(), None, None, 0.5, 0.5,
                                             1.0, 0.5, 0, 0, B, Cc, H, W, -100, ws.data_ptr(), ws.numel(), stream))

        def k_focal():
            ops.check(L.wsdl_focal_fwd_bwd(raw.data_ptr(), masks.data_ptr(), loss.data_ptr(), dl.data_ptr(), inv.data_ptr(), B, Cc, H, W, 2.0,
                                           -100, None, None, 0, ws.data_ptr(), ws.numel(), stream))

        def k_ce():
            ops.check(L.wsdl_softmax_ce_ex_fwd_bwd(raw.data_ptr(), masks.data_ptr(), loss.data_ptr(), dl.data_ptr(), inv.data_ptr(), B, Cc, H,
                                                   W, 1.0, -100, None, pw.data_ptr(), 0.0, 0, ws.data_ptr(), ws.numel(), stream))
        bytes_tv, bytes_fo, bytes_ce = n * (2 * (4 * Cc + 8) + 4 * Cc), n * (4 * Cc + 8 + 4 * Cc), n * (4 * Cc + 8 + 4 + 4 * Cc)
        dice, focal, plain = wnn.DiceLoss(), wnn.FocalLoss(), wnn.CrossEntropyLoss()
        both = wnn.CrossEntropyTverskyLoss(lam=1.0, alpha=0.3, beta=0.7).to(dev)

        def fwd_bwd(crit):
            logits.grad = None
            crit(logits, masks).backward()

        def torch_dice():
            logits.grad = None
            s = torch.softmax(logits, dim=1)
            y = F.one_hot(masks, Cc).permute(0, 3, 1, 2).to(s.dtype)
            inter, p, yy = (s * y).sum(dim=(0, 2, 3)), s.sum(dim=(0, 2, 3)), y.sum(dim=(0, 2, 3))
            (1 - (2 * inter + 1.0) / (p + yy + 1.0)).mean().backward()

        def torch_focal():
            logits.grad = None
            lsy = torch.log_softmax(logits, dim=1).gather(1, masks[:, None])[:, 0]
            ((1 - lsy.exp()) ** 2.0 * -lsy).mean().backward()
        variants = [
            ("kernel: wsdl_tversky_fwd_bwd (C ABI, sums + finalize + gradient)", bytes_tv, k_tversky),
            ("kernel: wsdl_focal_fwd_bwd (C ABI, fused pass + finalize)", bytes_fo, k_focal),
            ("kernel: wsdl_softmax_ce_ex_fwd_bwd with a pixel weight (C ABI, fused pass + finalize)", bytes_ce, k_ce),
            ("criterion: wnn.DiceLoss forward + backward", 0, lambda: fwd_bwd(dice)),
            ("criterion: wnn.FocalLoss forward + backward", 0, lambda: fwd_bwd(focal)),
            ("criterion: wnn.CrossEntropyTverskyLoss forward + backward", 0, lambda: fwd_bwd(both)),
            ("criterion: wnn.CrossEntropyLoss forward + backward", 0, lambda: fwd_bwd(plain)),
            ("torch: soft Dice (softmax, one_hot, three sums, mean), forward + backward", 0, torch_dice),
            ("torch: focal (log_softmax, gather, exp, pow, mean), forward + backward", 0, torch_focal),
        ]
        agree = []
        for lib_fn, torch_fn in ((lambda: fwd_bwd(dice), torch_dice), (lambda: fwd_bwd(focal), torch_focal)):
            lib_fn()
            g_lib = logits.grad.clone()
            torch_fn()
            agree.append(((logits.grad - g_lib).abs().max() / g_lib.abs().max()).item())
        for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
            for _ in range(3):
                fn()
        rounds = [[time_round(torch, fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
        lines.append(f"logits ({B},{Cc},{H},{W}), K = {Cc}, {n} pixels; Tversky {bytes_tv / 1e6:.1f} MB, focal {bytes_fo / 1e6:.1f} MB, cross entropy "
                     f"{bytes_ce / 1e6:.1f} MB algorithmic; max |torch gradient - library gradient| / max |gradient|: Dice {agree[0]:.1e}, focal {agree[1]:.1e}:")
        means, spreads = [], []
        for i, (name, nbytes, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            mean = sum(t) / len(t)
            means.append(mean)
            spreads.append(max(t) - min(t))
            rate = f"{nbytes / mean / 1e3:8.1f} GB/s" if nbytes else ""
            lines.append(f"  {name:92s} {mean:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})  {rate}")
        lines.append(f"  the Tversky triple takes {means[0] / means[2]:.2f}x of the cross-entropy kernel at {bytes_tv / bytes_ce:.3f}x of its bytes, the focal "
                     f"pair {means[1] / means[2]:.2f}x at {bytes_fo / bytes_ce:.3f}x (run-to-run spreads {spreads[0]:.2f}, {spreads[1]:.2f} and {spreads[2]:.2f} us); "
                     f"the torch formulation takes {means[7] / means[3]:.2f}x of wnn.DiceLoss and {means[8] / means[4]:.2f}x of wnn.FocalLoss; "
                     f"wnn.CrossEntropyTverskyLoss takes {means[5] / means[6]:.2f}x of wnn.CrossEntropyLoss (+{means[5] - means[6]:.1f} us)")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
