#!/usr/bin/env python3
"""Timing of the prototype ops (csrc/prototype.hip) at features (16,448,32,32), (8,448,64,64) and (16,2048,16,16), K = 2 and 21.

Per shape and K, each entry point of the C ABI (called through ctypes on buffers made once, so a line is the library's launches
and nothing else) against the same contract written with torch ops in float32 on the same device:
  pool        wsdl_proto_pool (3 launches), per-image unit-vector prototypes | F.normalize + one-hot einsum + division
  similarity  wsdl_proto_similarity (2 launches), softmax activation         | F.normalize x 2 + einsum + softmax
  contrast    wsdl_proto_contrast with the gradient buffer (3 launches), and ops.prototype_contrast_loss + backward (the two
              launches that apply the upstream gradient on top)              | F.normalize + einsum + F.cross_entropy, forward + backward
  bank        wsdl_proto_ema (1 launch)                                      | torch.where on the masses
beside a plain device copy of the same feature tensor (the rate a pass over the features can reach).  Then one ``prototype_cam`` call
at images (16,3,256,256) with the network left out (its features are a fixed (16,448,32,32) tensor) beside ``ops.pamr`` and the walk of
``affinity_cam`` (256 steps, radius 5) on the same CAM.
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds after a warm-up of every variant,
min .. max beside the mean.  No ratio is fixed in advance: the file records what was measured.  Also recorded: registers, LDS and
scratch of every kernel of the file as the compiler reports them (needs hipcc; ``--no-resources`` leaves the section out).
Writes profiles/prototype_bench.txt (``--out`` elsewhere)."""
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
from weaklysuperviseddl_amd._lib import check, lib  # noqa: E402

SHAPES = ((16, 448, 32, 32), (8, 448, 64, 64), (16, 2048, 16, 16))
CLASSES = (2, 21)
T = 0.1


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def torch_pool(f, labels, K):
    u = F.normalize(f, dim=1)
    m = F.one_hot(labels, K).to(f.dtype)                                   # (B,h,w,K)
    mass = m.sum(dim=(1, 2))
    return torch.einsum("bdhw,bhwk->bkd", u, m) / mass.clamp_min(1)[..., None], mass


def torch_similarity(f, proto):
    return (torch.einsum("bdhw,bkd->bkhw", F.normalize(f, dim=1), F.normalize(proto, dim=2)) / T).softmax(dim=1)


def torch_loss(f, proto, labels):
    return F.cross_entropy(torch.einsum("bdhw,bkd->bkhw", F.normalize(f, dim=1), F.normalize(proto, dim=2)) / T, labels)


def variants_for(shape, K, dev):
    B, D, h, w = shape
    g = torch.Generator(device=dev).manual_seed(B * 1000 + D + K)
    f = torch.randn(B, D, h, w, device=dev, generator=g)
    labels = torch.randint(0, K, (B, h, w), device=dev, generator=g)
    copy = torch.empty_like(f)
    proto, mass = torch.empty(B, K, D, device=dev), torch.empty(B, K, device=dev)
    sim, dfeat = torch.empty(B, K, h, w, device=dev), torch.empty_like(f)
    loss, inv = torch.empty((), device=dev), torch.empty(1, device=dev)
    bank, count = torch.zeros(K, D, device=dev), torch.zeros(K, dtype=torch.int64, device=dev)
    nbytes = lib().wsdl_proto_workspace(B, D, K, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def pool():
        check(lib().wsdl_proto_pool(p(f), p(labels), None, p(proto), p(mass), B, D, h, w, K, 1, 1, 255, 1e-12, p(ws), nbytes, s))

    def similarity():
        check(lib().wsdl_proto_similarity(p(f), p(proto), None, p(sim), B, D, h, w, K, B, 2, T, 1e-12, p(ws), nbytes, s))

    def contrast():
        check(lib().wsdl_proto_contrast(p(f), p(proto), p(labels), None, None, p(loss), p(dfeat), p(inv), B, D, h, w, K, B, 255, T, 1e-12, 0,
                                        p(ws), nbytes, s))

    def ema():
        check(lib().wsdl_proto_ema(p(bank), p(count), p(proto), p(mass), K, D, 0.99, s))

    fg, ft = f.clone().requires_grad_(), f.clone().requires_grad_()

    def op_loss():
        fg.grad = None
        ops.prototype_contrast_loss(fg, proto, labels, temperature=T).backward()

    def t_loss():
        ft.grad = None
        torch_loss(ft, proto, labels).backward()

    def t_ema():
        bank.copy_(torch.where((mass[0] > 0)[:, None], torch.where((count == 0)[:, None], proto[0], 0.99 * bank + 0.01 * proto[0]), bank))
        count.add_((mass[0] > 0).long())
    pool()
    tp, tm = torch_pool(f, labels, K)
    checks = [f"max |torch float32 - device|: prototypes {(tp - proto).abs().max().item():.1e}, mass {(tm - mass).abs().max().item():.1e}"]
    similarity()
    checks.append(f"similarity {(torch_similarity(f, proto) - sim).abs().max().item():.1e}")
    op_loss()
    t_loss()
    checks.append(f"loss gradient {(fg.grad - ft.grad).abs().max().item():.1e} (largest {fg.grad.abs().max().item():.1e})")
    feat_bytes, px = 4.0 * B * D * h * w, B * h * w
    return [
        ("device copy of the features (torch copy_)", 2 * feat_bytes, lambda: copy.copy_(f)),
        ("pool: wsdl_proto_pool (3 launches)", feat_bytes + 8.0 * px + 4.0 * B * K * D, pool),
        ("pool, torch normalize + one-hot einsum float32", 0, lambda: torch_pool(f, labels, K)),
        ("similarity: wsdl_proto_similarity, softmax (2 launches)", feat_bytes + 4.0 * px * K, similarity),
        ("similarity, torch normalize + einsum + softmax float32", 0, lambda: torch_similarity(f, proto)),
        ("contrast: wsdl_proto_contrast, loss + gradient (3 launches)", 2 * feat_bytes + 8.0 * px, contrast),
        ("contrast: ops.prototype_contrast_loss + backward (3 + 2 launches)", 0, op_loss),
        ("contrast, torch normalize + einsum + cross_entropy, forward + backward", 0, t_loss),
        ("bank: wsdl_proto_ema (1 launch)", 12.0 * K * D, ema),
        ("bank, torch where float32", 0, t_ema),
    ], checks


def cam_variants(dev):
    from weaklysuperviseddl_amd.TraditionalModel.PsuedoMasks import prototype_cam
    g = torch.Generator(device=dev).manual_seed(7)
    images = torch.rand(16, 3, 256, 256, device=dev, generator=g)
    cam = torch.rand(16, 256, 256, device=dev, generator=g)
    feat = torch.randn(16, 448, 32, 32, device=dev, generator=g)
    small = ops.bilinear_resize(cam[:, None].contiguous(), (32, 32))
    return [
        ("prototype_cam, images (16,3,256,256), features (16,448,32,32) given", 0, lambda: prototype_cam(images, cam, lambda x: feat)),
        ("ops.pamr on the same CAM (10 iterations)", 0, lambda: ops.pamr(images, cam[:, None])),
        ("affinity_cam's walk: ops.affinity_random_walk, radius 5, 256 steps", 0,
         lambda: ops.affinity_random_walk(feat, small, radius=5, beta=8.0, num_iter=256)),
    ]


def kernel_resources():
    """(name, VGPRs, AGPRs, scratch bytes per lane, LDS bytes, waves per SIMD) of every kernel of csrc/prototype.hip."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "prototype.hip")
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


def measure(variants, reps, rounds, lines):
    for _name, _b, fn in variants:              # warm up every variant: code objects load at the first launch
        fn()
    times = [[time_round(fn, reps) for _name, _b, fn in variants] for _ in range(rounds)]
    means = []
    for i, (name, nbytes, _fn) in enumerate(variants):
        t = [r[i] for r in times]
        means.append(sum(t) / len(t))
        rate = f"  {nbytes / means[-1] / 1e6:6.3f} TB/s algorithmic" if nbytes else ""
        lines.append(f"  {name:76s} {means[-1]:10.2f} us ({min(t):10.2f} .. {max(t):10.2f}){rate}")
    spread = max((max(r[i] for r in times) - min(r[i] for r in times)) / means[i] for i in range(len(variants)))
    return means, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prototype_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prototype_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/prototype_bench.py on {torch.cuda.get_device_name(0)}: per-image prototypes, temperature {T:g}; {args.reps} back-to-back "
             f"calls per round, {args.rounds} rounds after a warm-up, the variants alternating inside a round; us = mean (min .. max over the "
             "rounds)"]
    slower = []
    for shape in SHAPES:
        for K in CLASSES:
            variants, checks = variants_for(shape, K, dev)
            lines.append(f"features {shape}, {shape[0] * shape[2] * shape[3]} pixels, K = {K}:")
            lines.append("  checks: " + "; ".join(checks))
            m, spread = measure(variants, args.reps, args.rounds, lines)
            lines.append(f"  spread over the rounds: up to {spread * 100:.1f} % of a mean.  torch / device: pool {m[2] / m[1]:.1f}x, similarity "
                         f"{m[4] / m[3]:.1f}x, contrast {m[7] / m[6]:.1f}x (C ABI alone: {m[7] / m[5]:.1f}x), bank {m[9] / m[8]:.1f}x; a copy of the "
                         f"features takes {m[0]:.1f} us.")
            slower += [f"{variants[d][0]} at {shape} K={K}" for d, t in ((1, 2), (3, 4), (6, 7), (8, 9)) if m[d] >= m[t]]
    lines.append("Kernels not faster than their torch formulation: " + ("; ".join(slower) if slower else "none") + ".")
    lines.append("prototype_cam beside the other refiners, CAM (16,256,256):")
    measure(cam_variants(dev), max(2, args.reps // 5), args.rounds, lines)
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The inputs are reused call after call and fit the last-level cache: TB/s are "
                 "algorithmic bytes (features read once, results written once; the contrast reads the features and writes their gradient) "
                 "over time, not HBM rates.")
    if not args.no_resources:
        lines.append("Kernel resources as the compiler reports them (gfx950, -O3): VGPRs, AGPRs, scratch bytes per lane, LDS bytes per "
                     "workgroup, waves per SIMD")
        for row in kernel_resources():
            lines.append("  %-36s %4s %4s %5s %6s %2s" % row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
