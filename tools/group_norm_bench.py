#!/usr/bin/env python3
"""Timing of GroupNorm (csrc/group_norm.hip) through the C ABI - forward (3 launches) and forward + complete backward (6) - at
IRN's head shapes, each with and without the fused ReLU, against ``torch.nn.functional.group_norm`` (+ ``relu``) and its autograd
on the same device (a native kernel of the tensor library) and against the bytes the passes move at the copy rate measured on
a tensor of the same size.  Three rounds, the variants alternating inside a round, the spread over the rounds beside every mean;
then registers, LDS and scratch of every kernel as the compiler reports them (needs hipcc; ``--no-resources`` leaves the section
out).  Writes profiles/group_norm_bench.txt (``--out`` elsewhere); what the file holds below the marker line is kept verbatim."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from weaklysuperviseddl_amd import ops  # noqa: E402

# (B, C, H, W), G
SHAPES = (((16, 32, 64, 64), 4), ((8, 32, 128, 128), 4), ((16, 160, 64, 64), 32))
EPS = 1e-5
RECORD_MARKER = "==== recorded beside the run above, NOT written by it"
# bytes per element the passes read and write (x twice and y once forward; backward: x and dy twice, dx once, y twice under relu)
FWD_BYTES, BWD_BYTES, BWD_RELU_BYTES = 12, 20, 28


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def variants_for(shape, G, relu, dev):
    B, C, H, W = shape
    HW, n = H * W, B * C * H * W
    g = torch.Generator(device=dev).manual_seed(B * C + G)
    x = torch.randn(shape, device=dev, generator=g) * 2.0 + 3.0
    dy = torch.randn(shape, device=dev, generator=g)
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.randn(C, device=dev, generator=g) * 0.5
    y, dx, spare = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    stats = torch.empty(2, B * G, device=dev, dtype=torch.float64)
    lib, P, S = ops.lib(), ops._p, ops._stream
    ws = ops.workspace(lib.wsdl_group_norm_workspace(B, C, HW, G), dev)

    def fwd():
        ops.check(lib.wsdl_group_norm_fwd(P(x), P(gamma), P(beta), P(y), P(stats[0]), P(stats[1]), B, C, HW, G, EPS, int(relu), P(ws),
                                          ws.numel(), S()))

    def bwd():
        ops.check(lib.wsdl_group_norm_bwd(P(x), P(dy), P(y) if relu else None, P(gamma), P(stats[0]), P(stats[1]), P(dx), P(dgamma),
                                          P(dbeta), B, C, HW, G, int(relu), 0, P(ws), ws.numel(), S()))

    def both():
        fwd()
        bwd()
    xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()

    def torch_fwd():
        with torch.no_grad():
            out = F.group_norm(xt, G, gt, bt, EPS)
            return F.relu(out) if relu else out

    def torch_both():
        out = F.group_norm(xt, G, gt, bt, EPS)
        out = F.relu(out) if relu else out
        return torch.autograd.grad(out, (xt, gt, bt), dy)
    both()
    ty, (tdx, tdg, tdb) = torch_fwd(), torch_both()
    checks = (f"max |torch float32 - device|: y {(ty - y).abs().max().item():.1e}, dx {(tdx - dx).abs().max().item():.1e}, dgamma "
              f"{(tdg - dgamma).abs().max().item():.1e} (largest {dgamma.abs().max().item():.1e}), dbeta {(tdb - dbeta).abs().max().item():.1e}")
    tag = " + relu" if relu else ""
    variants = [
        (f"forward{tag}: wsdl_group_norm_fwd (3 launches)", FWD_BYTES * n, fwd),
        (f"forward{tag}, torch F.group_norm{' + F.relu' if relu else ''}", 0, torch_fwd),
        (f"forward + backward{tag}: wsdl_group_norm_fwd + _bwd (6 launches)", (FWD_BYTES + (BWD_RELU_BYTES if relu else BWD_BYTES)) * n, both),
        (f"forward + backward{tag}, torch with autograd.grad wrt x, weight, bias", 0, torch_both),
        ("copy of a tensor of this size (torch copy_)", 8 * n, lambda: spare.copy_(x)),
    ]
    return variants, checks


def kernel_resources():
    """(name, VGPRs, AGPRs, scratch bytes per lane, LDS bytes, waves per SIMD) of every kernel of csrc/group_norm.hip."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "group_norm.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", os.path.join(tmp, "a.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*(.+?): (\S+) \[-Rpass-analysis", line) or re.search(r"remark: \s*(.+?): (\S+) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    filt = shutil.which("c++filt")
    out = []
    for row in rows:
        name = row["name"]
        if filt:
            name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::|^void |\(.*$", "", name)
        out.append((name, row.get("VGPRs", "?"), row.get("AGPRs", "?"), row.get("ScratchSize [bytes/lane]", "?"),
                    row.get("LDS Size [bytes/block]", "?"), row.get("Occupancy [waves/SIMD]", "?")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_norm_bench.txt"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_norm_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/group_norm_bench.py on {torch.cuda.get_device_name(0)}: eps {EPS:g}; {args.reps} back-to-back calls per round after a "
             f"warm-up call, {args.rounds} rounds, the variants alternating inside a round; us = mean (min .. max over the rounds)"]
    for shape, G in SHAPES:
        for relu in (False, True):
            variants, checks = variants_for(shape, G, relu, dev)
            for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
                fn()
            rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
            n = shape[0] * shape[1] * shape[2] * shape[3]
            lines.append(f"x {shape}, {G} groups of {shape[1] // G} channels ({shape[0] * G} groups of {n // (shape[0] * G)} floats, {4 * n / 1e6:.1f} MB), "
                         f"relu {relu}:")
            lines.append("  checks: " + checks)
            means = [sum(r[i] for r in rounds) / len(rounds) for i in range(len(variants))]
            copy_rate = variants[-1][1] / means[-1] / 1e6            # TB/s
            for i, (name, nbytes, _fn) in enumerate(variants):
                t = [r[i] for r in rounds]
                rate = ""
                if nbytes:
                    rate = f"  {nbytes / means[i] / 1e6:6.3f} TB/s of pass bytes"
                    if i != len(variants) - 1:
                        rate += f"; those bytes at the copy rate: {nbytes / copy_rate / 1e6:7.2f} us = {nbytes / copy_rate / 1e6 / means[i] * 100:5.1f} %"
                lines.append(f"  {name:74s} {means[i]:9.2f} us ({min(t):9.2f} .. {max(t):9.2f}){rate}")
            spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(len(variants)))
            lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  torch / device: forward {means[1] / means[0]:.2f}x, "
                         f"forward + backward {means[3] / means[2]:.2f}x.")
            torch.cuda.empty_cache()
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The tensors are reused call after call and fit the last-level cache, the copy too: "
                 f"TB/s are pass bytes ({FWD_BYTES} B per element forward: x twice, y once; {BWD_BYTES} backward: x and dy twice, dx once; "
                 f"{BWD_RELU_BYTES} under relu: y twice more) over time, not HBM rates.")
    if not args.no_resources:
        lines.append("Kernel resources as the compiler reports them (gfx950, -O3; compiled apart from the timed run): VGPRs, AGPRs, scratch "
                     "bytes per lane, LDS bytes per workgroup, waves per SIMD")
        for row in kernel_resources():
            lines.append("  %-44s %4s %4s %5s %6s %2s" % row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):
        old = open(args.out).read()
        if RECORD_MARKER in old:
            text += old[old.index(RECORD_MARKER):]
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
