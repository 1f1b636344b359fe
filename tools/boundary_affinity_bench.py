#!/usr/bin/env python3
"""Timing of the IRN boundary-path ops (csrc/boundary_affinity.hip) at boundary maps (16,64,64) and (8,128,128), radius 5 (P = 34
pairs, 242 path points) and, for the record, radius 8 (P = 96, 1078 points).

Per shape and radius, through the C ABI on preallocated buffers:
  forward      wsdl_path_affinity with the arg plane: one launch
  backward     wsdl_path_affinity_backward: one launch
  loss         wsdl_path_affinity_loss with its gradient: five launches
and through ops (the walk is a sequence of C ABI calls):
  walk         ops.edge_random_walk, beta 10, 256 steps, C = 1 and C = 2 (radius 5 only)
each against the same contract written with torch ops in float32 on the device - IRN's own formulation: the map padded with 1
(logits: with 0, the kinds mask the invalid pairs), an index gather of every path's points, ``amax`` over the path; torch's
autograd for the gradients; the transitions and the stencil walk of tools/affinity_bench.py for the walk.
Device-event times over back-to-back calls after a warm-up, the variants alternating inside a round, three rounds, min .. max
beside the mean.  No ratio is fixed in advance: the file records what was measured.  Also recorded: registers, LDS and scratch of
every kernel of the file as the compiler reports them (needs hipcc; ``--no-resources`` leaves the section out).
Writes profiles/boundary_affinity_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import weaklysuperviseddl_amd  # noqa: E402
from weaklysuperviseddl_amd import ops  # noqa: E402
from weaklysuperviseddl_amd._lib import check  # noqa: E402
from affinity_bench import TorchAffinity, time_round  # noqa: E402

SHAPES = ((16, 64, 64), (8, 128, 128))
RADII = (5, 8)
BETA, STEPS = 10.0, 256
# profiles/boundary_affinity_bench.txt also holds what this tool does not measure (the gather kernel's first form, bench.py against
# the parent commit, what bounds each kernel).  Everything from this marker line on is kept as it is when the tool rewrites the file.
RECORD_MARKER = "==== recorded beside the run above, NOT written by it (kept verbatim by tools/boundary_affinity_bench.py) ===="


class TorchPaths:
    """The contract with the tensor library's own kernels, float32, on the device: gather of the path points and amax."""

    def __init__(self, h, w, radius, dev):
        self.r, self.h, self.w = radius, h, w
        self.offs, paths = ops.affinity_offsets(radius), ops.affinity_paths(radius)
        longest = max(len(p) for p in paths)
        pw = w + 2 * (radius - 1)
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        idx = torch.empty(len(paths), longest, h, w, dtype=torch.int64)
        for j, path in enumerate(paths):
            for t in range(longest):
                y, x = path[t] if t < len(path) else path[0]            # (a repeated point does not change the maximum)
                idx[j, t] = (yy + y) * pw + (xx + x + radius - 1)
        self.idx = idx.view(-1).to(dev)
        self.shape = (len(paths), longest, h, w)
        self.kinds_of = TorchAffinity(h, w, radius)

    def path_max(self, e, pad):
        r = self.r
        padded = F.pad(e, (r - 1, r - 1, 0, r - 1), value=pad)
        return padded.flatten(1)[:, self.idx].view(e.shape[0], *self.shape).amax(dim=2)

    def affinity(self, e):
        return 1 - self.path_max(e, 1.0)

    def loss(self, z, labels, weights=(0.25, 0.25, 0.5), eps=1e-5):
        zmax, k = self.path_max(z, 0.0), self.kinds_of.kinds(labels).float()
        n = k.flatten(1).sum(dim=1)
        pos, neg = -torch.log(torch.sigmoid(-zmax) + eps), -torch.log(torch.sigmoid(zmax) + eps)
        return weights[0] * (pos * k[0]).sum() / (n[0] + eps) + weights[1] * (pos * k[1]).sum() / (n[1] + eps) + \
            weights[2] * (neg * k[2]).sum() / (n[2] + eps)

    def walk(self, e, m, beta, steps):
        trans = self.kinds_of.transitions(self.affinity(e), beta)
        return self.kinds_of.walk(trans, m * (1 - e[:, None]), steps)


def variants_for(shape, radius, dev, with_walk):
    B, h, w = shape
    lib = weaklysuperviseddl_amd.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    e = torch.rand(B, h, w, device=dev, generator=g)
    e[:, 1:] = 0.5 * e[:, 1:] + 0.5 * e[:, :-1]
    e = e.contiguous()
    z = torch.logit(e.clamp(1e-3, 1 - 1e-3)).contiguous()
    labels = torch.tensor([0, 1, 2, 255], device=dev)[torch.randint(0, 4, (B, (h + 3) // 4, (w + 3) // 4), device=dev, generator=g)]
    labels = labels.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w].contiguous()
    tp = TorchPaths(h, w, radius, dev)
    P, points = len(tp.offs), sum(len(p) for p in ops.affinity_paths(radius))
    n = B * h * w
    aff = torch.empty(B, P, h, w, device=dev)
    arg = torch.empty(B, P, h, w, device=dev, dtype=torch.uint8)
    daff = torch.randn(B, P, h, w, device=dev, generator=g)
    dedge, dz, loss = torch.empty(B, h, w, device=dev), torch.empty(B, h, w, device=dev), torch.empty((), device=dev)
    ws = torch.empty(lib.wsdl_path_affinity_workspace(B, h, w, radius), device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream

    def forward():
        check(lib.wsdl_path_affinity(e.data_ptr(), B, h, w, radius, aff.data_ptr(), arg.data_ptr(), stream))

    def backward():
        check(lib.wsdl_path_affinity_backward(daff.data_ptr(), arg.data_ptr(), dedge.data_ptr(), B, h, w, radius, stream))

    def fused_loss():
        check(lib.wsdl_path_affinity_loss(z.data_ptr(), labels.data_ptr(), loss.data_ptr(), dz.data_ptr(), None, B, h, w, radius, 255, 0.25,
                                          0.25, 0.5, 1e-5, ws.data_ptr(), ws.numel(), stream))
    et, zt = e.clone().requires_grad_(), z.clone().requires_grad_()
    at = tp.affinity(et)

    def torch_backward():
        torch.autograd.grad(at, et, daff, retain_graph=True)

    def torch_loss():
        zt.grad = None
        tp.loss(zt, labels).backward()
    forward()
    backward()
    fused_loss()
    torch_loss()
    checks = [f"max |torch float32 - device|: affinities {(tp.affinity(e) - aff).abs().max().item():.1e}",
              f"backward {(torch.autograd.grad(at, et, daff, retain_graph=True)[0] - dedge).abs().max().item():.1e} "
              f"(largest {dedge.abs().max().item():.1e})",
              f"loss {abs(tp.loss(z, labels).item() - loss.item()):.1e}, its gradient {(zt.grad - dz).abs().max().item():.1e} "
              f"(largest {dz.abs().max().item():.1e})"]
    variants = [
        ("forward: wsdl_path_affinity with arg (1 launch)", n * (4.0 + 5.0 * P), 4.0 * n * points, forward),
        ("forward, torch gather + amax float32", 0, 0, lambda: tp.affinity(e)),
        ("backward: wsdl_path_affinity_backward (1 launch)", n * (4.0 + 5.0 * P), 0, backward),
        ("backward, torch autograd of gather + amax", 0, 0, torch_backward),
        ("loss + gradient: wsdl_path_affinity_loss (5 launches)", n * (16.0 + 10.0 * P), 4.0 * n * points, fused_loss),
        ("loss + gradient, torch gather + amax and autograd float32", 0, 0, torch_loss),
    ]
    walks = {}
    if with_walk:
        for C in (1, 2):
            m = torch.rand(B, C, h, w, device=dev, generator=g)
            out = torch.empty_like(m)
            a = ops.edge_random_walk(e, m, radius=radius, beta=BETA, num_iter=STEPS)
            checks.append(f"walk C={C}: torch formulation {(tp.walk(e, m, BETA, STEPS) - a).abs().max().item():.1e}")
            walks[C] = len(variants)
            variants += [
                (f"walk C={C}: ops.edge_random_walk, {STEPS} steps (3 + {STEPS} launches)", 0, 0,
                 lambda m=m, out=out: ops.edge_random_walk(e, m, radius=radius, beta=BETA, num_iter=STEPS, out=out)),
                (f"walk C={C}, torch formulation float32, {STEPS} x {2 * P + 1} slice products", 0, 0, lambda m=m: tp.walk(e, m, BETA, STEPS)),
            ]
    return variants, checks, walks


def kernel_resources():
    """(name, VGPRs, AGPRs, scratch bytes per lane, LDS bytes, waves per SIMD) of every kernel of csrc/boundary_affinity.hip."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "boundary_affinity.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_affinity_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_affinity_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/boundary_affinity_bench.py on {torch.cuda.get_device_name(0)}: beta {BETA:g}, {STEPS} walk steps; {args.reps} back-to-back "
             f"calls per round after a warm-up call (torch walk: 2), {args.rounds} rounds, the variants alternating inside a round; us = mean "
             "(min .. max over the rounds)"]
    for shape in SHAPES:
        for radius in RADII:
            variants, checks, walks = variants_for(shape, radius, dev, with_walk=radius == 5)
            reps = [2 if "torch formulation" in name else args.reps for name, _b, _l, _fn in variants]
            for _name, _b, _l, fn in variants:          # warm up every variant: code objects load at the first launch
                fn()
            rounds = [[time_round(fn, k) for (_name, _b, _l, fn), k in zip(variants, reps)] for _ in range(args.rounds)]
            n = shape[0] * shape[1] * shape[2]
            lines.append(f"boundary map {shape}, {n} pixels, radius {radius} (P = {len(ops.affinity_offsets(radius))}, "
                         f"{sum(len(p) for p in ops.affinity_paths(radius))} path points):")
            lines.append("  checks: " + "; ".join(checks))
            means = []
            for i, (name, nbytes, lds, _fn) in enumerate(variants):
                t = [r[i] for r in rounds]
                mean = sum(t) / len(t)
                means.append(mean)
                rate = f"  {nbytes / mean / 1e6:6.3f} TB/s algorithmic" if nbytes else ""
                rate += f", {lds / mean / 1e6:6.3f} TB/s of LDS reads" if lds else ""
                lines.append(f"  {name:78s} {mean:11.2f} us ({min(t):11.2f} .. {max(t):11.2f}){rate}")
            spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(len(variants)))
            lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  torch / device: forward {means[1] / means[0]:.1f}x, "
                         f"backward {means[3] / means[2]:.1f}x, loss + gradient {means[5] / means[4]:.1f}x.")
            for C, i in walks.items():
                lines.append(f"  walk C={C}: {means[i] / STEPS:.2f} us per step; the torch formulation takes {means[i + 1] / means[i]:.0f}x of it.")
            torch.cuda.empty_cache()
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The inputs are reused call after call and fit the last-level cache: TB/s are "
                 "algorithmic bytes (inputs read once, outputs written once; the loss: its workspace planes written and read once) over "
                 "time, not HBM rates; LDS reads are 4 bytes per path point and pixel.")
    if not args.no_resources:
        lines.append("Kernel resources as the compiler reports them (gfx950, -O3): VGPRs, AGPRs, scratch bytes per lane, LDS bytes per "
                     "workgroup, waves per SIMD")
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
