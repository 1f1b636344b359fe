#!/usr/bin/env python3
"""Timing of the AffinityNet ops (csrc/affinity.hip) at features (16,448,32,32) and (8,448,64,64), radius 5 (P = 34 pairs).

Per shape:
  forward      ops.pair_affinity: one launch; D * P abs-differences per pixel
  loss         ops.affinity_loss + backward: counts, forward with partial sums and pair coefficients, finalize, gradient, the
               scaling by the upstream gradient
  transitions  ops.affinity_transitions (beta 8)
  walk         ops.random_walk, 256 steps (one launch each), C = 2 and C = 21
each against the same contract written with torch ops in float32 on the device (shifted slices; for the loss torch's autograd of
them), and the walk also against PSA's own form on the device: the dense column-normalised (hw x hw) matrix per image squared eight
times (t = 2^8 = 256) and applied to the scores.
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds, min .. max beside the mean.
No ratio is fixed in advance: the file records what was measured.  Also recorded: registers, LDS and scratch of every kernel of
the file as the compiler reports them (needs hipcc; ``--no-resources`` leaves the section out).  A section of the output file
behind RECORD_MARKER (measurements of code that is no longer in the tree) is carried over unchanged.
Writes profiles/affinity_bench.txt (``--out`` elsewhere)."""
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
from weaklysuperviseddl_amd import ops  # noqa: E402

SHAPES = ((16, 448, 32, 32), (8, 448, 64, 64))
RADIUS, BETA, STEPS = 5, 8.0, 256


# profiles/affinity_bench.txt also holds the record of a measurement this tree cannot repeat (the walk's deleted second path).
# Everything from this marker line on is kept as it is when the tool rewrites the file; nothing below it is from the run above it.
RECORD_MARKER = "==== recorded earlier, NOT from the run above (kept verbatim by tools/affinity_bench.py) ===="


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def window(h, w, dy, dx):
    y1, x0, x1 = h - dy, max(0, -dx), min(w, w - dx)
    if y1 <= 0 or x1 <= x0:
        return None
    return slice(0, y1), slice(x0, x1), slice(dy, y1 + dy), slice(x0 + dx, x1 + dx)


class TorchAffinity:
    """The contract with the tensor library's own kernels, float32, on the device."""

    def __init__(self, h, w, radius):
        self.offs = ops.affinity_offsets(radius)
        self.win = [window(h, w, dy, dx) for dy, dx in self.offs]

    def affinity(self, f):
        B, D, h, w = f.shape
        out = torch.zeros(B, len(self.offs), h, w, device=f.device)
        for j, win in enumerate(self.win):
            if win is not None:
                ys, xs, yt, xt = win
                out[:, j, ys, xs] = torch.exp(-(f[:, :, ys, xs] - f[:, :, yt, xt]).abs().mean(dim=1))
        return out

    def kinds(self, labels, ignore=255):
        B, h, w = labels.shape
        k = torch.zeros(3, B, len(self.offs), h, w, dtype=torch.bool, device=labels.device)
        for j, win in enumerate(self.win):
            if win is not None:
                ys, xs, yt, xt = win
                a, b = labels[:, ys, xs], labels[:, yt, xt]
                ok = (a != ignore) & (b != ignore)
                k[0, :, j, ys, xs] = ok & (a == b) & (a == 0)
                k[1, :, j, ys, xs] = ok & (a == b) & (a > 0)
                k[2, :, j, ys, xs] = ok & (a != b)
        return k

    def loss(self, f, labels, weights=(0.25, 0.25, 0.5), eps=1e-5):
        a, k = self.affinity(f), self.kinds(labels).float()
        n = k.flatten(1).sum(dim=1)
        pos, neg = -torch.log(a + eps), -torch.log(1 + eps - a)
        return weights[0] * (pos * k[0]).sum() / (n[0] + eps) + weights[1] * (pos * k[1]).sum() / (n[1] + eps) + \
            weights[2] * (neg * k[2]).sum() / (n[2] + eps)

    def transitions(self, aff, beta):
        B, P, h, w = aff.shape
        pw = torch.zeros(B, 2 * P + 1, h, w, device=aff.device)
        pw[:, 0] = 1
        for j, win in enumerate(self.win):
            if win is not None:
                ys, xs, yt, xt = win
                v = aff[:, j, ys, xs] ** beta
                pw[:, 1 + 2 * j, ys, xs] = v
                pw[:, 2 + 2 * j, yt, xt] = v
        return pw / pw.sum(dim=1, keepdim=True)

    def walk(self, trans, m, steps):
        for _ in range(steps):
            out = trans[:, 0:1] * m
            for j, win in enumerate(self.win):
                if win is not None:
                    ys, xs, yt, xt = win
                    out[:, :, ys, xs] += trans[:, 1 + 2 * j:2 + 2 * j, ys, xs] * m[:, :, yt, xt]
                    out[:, :, yt, xt] += trans[:, 2 + 2 * j:3 + 2 * j, yt, xt] * m[:, :, ys, xs]
            m = out
        return m

    def dense_matrix(self, aff, beta):
        """PSA's (B, hw, hw) matrix: (A + I) ** beta, every column divided by its sum."""
        B, P, h, w = aff.shape
        n = h * w
        A = torch.zeros(B, n, n, device=aff.device)
        idx = torch.arange(n, device=aff.device).view(h, w)
        for j, win in enumerate(self.win):
            if win is not None:
                ys, xs, yt, xt = win
                p, q = idx[ys, xs].reshape(-1), idx[yt, xt].reshape(-1)
                v = aff[:, j, ys, xs].reshape(B, -1)
                A[:, p, q] = v
                A[:, q, p] = v
        T = (A + torch.eye(n, device=aff.device)) ** beta
        return T / T.sum(dim=1, keepdim=True)

    @staticmethod
    def dense_walk(T, m, logt):
        for _ in range(logt):
            T = torch.bmm(T, T)
        B, C, h, w = m.shape
        return torch.bmm(m.view(B, C, h * w), T).view(B, C, h, w)


def variants_for(shape, dev):
    B, D, h, w = shape
    g = torch.Generator(device=dev).manual_seed(0)
    f = torch.randn(B, D, h, w, device=dev, generator=g)
    f[:, :, 1:] = 0.6 * f[:, :, 1:] + 0.4 * f[:, :, :-1]
    f = f.contiguous()
    labels = torch.tensor([0, 1, 2, 255], device=dev)[torch.randint(0, 4, (B, (h + 3) // 4, (w + 3) // 4), device=dev, generator=g)]
    labels = labels.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w].contiguous()
    tp = TorchAffinity(h, w, RADIUS)
    P = len(tp.offs)
    fg, ft = f.clone().requires_grad_(), f.clone().requires_grad_()
    aff = ops.pair_affinity(f, RADIUS)
    trans = ops.affinity_transitions(aff, BETA, RADIUS)
    T = tp.dense_matrix(aff, BETA)
    checks = [f"max |torch float32 - device|: affinities {(tp.affinity(f) - aff).abs().max().item():.1e}",
              f"transitions {(tp.transitions(aff, BETA) - trans).abs().max().item():.1e}"]

    def device_loss():
        fg.grad = None
        ops.affinity_loss(fg, labels, radius=RADIUS).backward()

    def torch_loss():
        ft.grad = None
        tp.loss(ft, labels).backward()
    device_loss()
    torch_loss()
    checks.append(f"loss gradient {(fg.grad - ft.grad).abs().max().item():.1e} (largest {fg.grad.abs().max().item():.1e})")
    n = B * h * w
    variants = [
        ("forward: ops.pair_affinity (1 launch)", 4.0 * n * (D + P), lambda: ops.pair_affinity(f, RADIUS)),
        ("forward, torch slices float32", 0, lambda: tp.affinity(f)),
        ("loss + gradient: ops.affinity_loss, backward (5 + 1 launches)", 0, device_loss),
        ("loss + gradient, torch slices and autograd float32", 0, torch_loss),
        ("transitions: ops.affinity_transitions (1 launch)", 4.0 * n * (3 * P + 1), lambda: ops.affinity_transitions(aff, BETA, RADIUS)),
        ("transitions, torch slices float32", 0, lambda: tp.transitions(aff, BETA)),
    ]
    walks = {}
    for C in (2, 21):
        m = torch.rand(B, C, h, w, device=dev, generator=g)
        out = torch.empty_like(m)
        a = ops.random_walk(trans, m, STEPS, radius=RADIUS)
        dense = tp.dense_walk(T, m, 8)
        checks.append(f"walk C={C}: torch stencil {(tp.walk(trans, m, STEPS) - a).abs().max().item():.1e}, "
                      f"dense squaring {(dense - a).abs().max().item():.1e}")
        walks[C] = len(variants)
        variants += [
            (f"walk C={C}: {STEPS} steps ({STEPS} launches)", 0,
             lambda m=m, out=out: ops.random_walk(trans, m, STEPS, radius=RADIUS, out=out)),
            (f"walk C={C}, torch stencil float32, {STEPS} x {2 * P + 1} slice products", 0, lambda m=m: tp.walk(trans, m, STEPS)),
            (f"walk C={C}, PSA's dense form on the device: 8 squarings of ({h * w} x {h * w}) + 1 product", 0,
             lambda m=m: tp.dense_walk(T, m, 8)),
        ]
    return variants, checks, walks, lambda: tp.dense_matrix(aff, BETA)


def kernel_resources():
    """(name, VGPRs, AGPRs, scratch bytes per lane, LDS bytes, waves per SIMD) of every kernel of csrc/affinity.hip."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "affinity.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affinity_bench.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affinity_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/affinity_bench.py on {torch.cuda.get_device_name(0)}: radius {RADIUS} (P = 34), beta {BETA:g}, {STEPS} walk steps; "
             f"{args.reps} back-to-back calls per round (torch walk variants: 2), {args.rounds} rounds, the variants alternating inside a "
             "round; us = mean (min .. max over the rounds)"]
    for shape in SHAPES:
        variants, checks, walks, dense_build = variants_for(shape, dev)
        reps = [2 if "torch stencil" in name or "dense form" in name else args.reps for name, _b, _fn in variants]
        for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
            fn()
        rounds = [[time_round(fn, k) for (_name, _b, fn), k in zip(variants, reps)] for _ in range(args.rounds)]
        t_dense = [time_round(dense_build, 2) for _ in range(args.rounds)]
        lines.append(f"features {shape}, {shape[0] * shape[2] * shape[3]} pixels:")
        lines.append("  checks: " + "; ".join(checks))
        means = []
        for i, (name, nbytes, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            mean = sum(t) / len(t)
            means.append(mean)
            rate = f"  {nbytes / mean / 1e6:6.3f} TB/s algorithmic (inputs read once, outputs written once)" if nbytes else ""
            lines.append(f"  {name:86s} {mean:11.2f} us ({min(t):11.2f} .. {max(t):11.2f}){rate}")
        lines.append(f"  (building PSA's dense matrix from the affinities with torch ops, not in the dense line above: "
                     f"{sum(t_dense) / len(t_dense):.0f} us)")
        spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(len(variants)))
        lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  torch / device: forward {means[1] / means[0]:.1f}x, loss + "
                     f"gradient {means[3] / means[2]:.1f}x, transitions {means[5] / means[4]:.1f}x.")
        for C, i in walks.items():
            lines.append(f"  walk C={C}: {means[i] / STEPS:.2f} us per step; the torch stencil takes {means[i + 1] / means[i]:.0f}x and PSA's dense "
                         f"form {means[i + 2] / means[i]:.2f}x of it.")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The inputs are reused call after call and fit the last-level cache: TB/s are "
                 "algorithmic bytes over time, not HBM rates.")
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
