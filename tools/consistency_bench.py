"""The view-consistency kernels (csrc/consistency.hip) timed through the C ABI with device events; writes text lines to --out
(default profiles/consistency_bench.txt) and prints them, then one JSON line.  Three rounds after a warm-up, the variants of
a comparison alternating inside every round; us per call = mean (min .. max over the rounds).

Shapes (B,C,H,W): (16,2,256,256) and (8,21,512,512); the teacher has the student's size, the rows are drawn by
Augment(scale=(0.5, 2), rotate=30, hflip=0.5) - the magnifications the adjoint is built for.  Four comparisons:
  1. the fused loss (kl, normalize = all, forward + gradient) against the same contract in the tensor library's ops on the
     device: F.grid_sample(border) + softmax + confidence mask + KL, forward + backward;
  2. the fused loss against the unfused pair wsdl_warp_scores_fwd + wsdl_consistency_fwd_bwd without rows;
  3. the fused loss against the cross-entropy kernel (wsdl_softmax_ce_fwd_bwd) - logits in, gradient out, no teacher: the
     bytes the loss cannot avoid;
  4. the adjoint wsdl_warp_scores_bwd against torch autograd's backward of grid_sample.
--resources-only compiles consistency.hip with -Rpass-analysis=kernel-resource-usage and writes the table of registers, LDS and
scratch per kernel instantiation (no device needed); a timing run includes the table when the file is there."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESOURCES = os.path.join(ROOT, "profiles", "consistency_resources.txt")


def resource_table():
    from weaklysuperviseddl_amd import _build
    src = os.path.join(_build.CSRC, "consistency.hip")
    cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            name = re.sub(r"\(anonymous namespace\)::|\(.*$|^void ", "", name)
            cur = {"kernel": name}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    out = ["kernel resources of csrc/consistency.hip (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage);",
           "consistency_kernel<NC, MODE>: NC = classes held in registers (0: any C, re-read per pass), MODE 0 fused / 1 sums / 2 gradient",
           f"  {'kernel':44s} {'VGPRs':>5s} {'AGPRs':>5s} {'SGPRs':>5s} {'LDS B':>6s} {'scratch B/lane':>14s} {'waves/SIMD':>10s}"]
    for r in rows:
        out.append(f"  {r['kernel']:44s} {r.get('VGPRs', '?'):>5s} {r.get('AGPRs', '0'):>5s} {r.get('TotalSGPRs', '?'):>5s} "
                   f"{r.get('LDS', '?'):>6s} {r.get('ScratchSize', '?'):>14s} {r.get('Occupancy', '?'):>10s}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.txt"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        lines = resource_table()
        with open(RESOURCES, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench: needs a GPU (nothing is measured without one)")
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd._lib import check, lib
    from weaklysuperviseddl_amd.augment import Augment
    dev = torch.device("cuda:0")
    L = lib()
    stream = ops.raw_stream(dev)
    lines, res = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps

    def compare(title, variants, nbytes=None):
        times = {n: [] for n, _ in variants}
        for _ in range(a.rounds):
            for n, fn in variants:
                times[n].append(timed(fn))
        base = sum(times[variants[0][0]]) / a.rounds
        say(f"  {title}")
        for n, _ in variants:
            t = times[n]
            mean = sum(t) / len(t)
            rate = "" if nbytes is None else f"  {nbytes / mean / 1e6:5.2f} TB/s of its own bytes"
            say(f"    {n:52s} {mean:9.2f} us ({min(t):.2f} .. {max(t):.2f})  x{mean / base:.2f}{rate}")
            res[f"{title}/{n}"] = {"us": round(mean, 3), "min": round(min(t), 3), "max": round(max(t), 3)}
        return {n: sum(t) / len(t) for n, t in times.items()}

    say(f"tools/consistency_bench.py on {torch.cuda.get_device_name(0)}: {a.steps} calls per round after {a.warmup} warm-up calls, "
        f"{a.rounds} rounds; us per call = mean (min .. max over the rounds); x = ratio to the first line of a comparison")
    if os.path.exists(RESOURCES):
        with open(RESOURCES) as f:
            for line in f.read().splitlines():
                say(line)
    verdicts = []
    for (B, Cc, H, W) in ((16, 2, 256, 256), (8, 21, 512, 512)):
        g = torch.Generator().manual_seed(B)
        z = torch.randn(B, Cc, H, W, generator=g).to(dev)
        t = (3.0 * torch.randn(B, Cc, H, W, generator=g)).to(dev)
        rows = Augment(scale=(0.5, 2.0), rotate=30.0, hflip=0.5).draw(B, (H, W), (H, W), g).to(dev)
        labels = torch.randint(0, Cc, (B, H, W), generator=g).to(dev)
        knobs = torch.tensor([0.7, 1.0, 1.0], device=dev)
        loss, dz = torch.empty((), device=dev), torch.empty_like(z)
        inv = torch.empty(1, device=dev)
        warped, dsrc = torch.empty_like(t), torch.empty_like(t)
        ws = torch.empty(L.wsdl_consistency_workspace(), dtype=torch.uint8, device=dev)
        ws_ce = torch.empty(L.wsdl_reduce_workspace(), dtype=torch.uint8, device=dev)
        P = lambda x: x.data_ptr()                                         # noqa: E731

        def fused(normalize=0):
            check(L.wsdl_consistency_fwd_bwd(P(z), P(t), P(rows), None, P(knobs), B, Cc, H, W, H, W, 0, 0, normalize, 0, P(loss), P(dz),
                                             None, None, None, P(ws), ws.numel(), stream))

        def unfused():
            check(L.wsdl_warp_scores_fwd(P(t), P(rows), B, Cc, H, W, H, W, 0, float("nan"), 0, P(warped), None, stream))
            check(L.wsdl_consistency_fwd_bwd(P(z), P(warped), None, None, P(knobs), B, Cc, H, W, H, W, 0, 0, 0, 0, P(loss), P(dz), None,
                                             None, None, P(ws), ws.numel(), stream))

        def ce():
            check(L.wsdl_softmax_ce_fwd_bwd(P(z), P(labels), P(loss), P(dz), P(inv), B, Cc, H, W, 1.0, -100, P(ws_ce), ws_ce.numel(),
                                            stream))

        def adjoint():
            check(L.wsdl_warp_scores_bwd(P(z), P(rows), B, Cc, H, W, H, W, 0, 0, P(dsrc), stream))

        # the tensor library's version of the same contract: the sampling grid is made once, outside the timed region
        u = torch.arange(W, device=dev, dtype=torch.float32) + 0.5
        v = torch.arange(H, device=dev, dtype=torch.float32) + 0.5
        xs = rows[:, 0, None, None] * u[None, None, :] + rows[:, 1, None, None] * v[None, :, None] + rows[:, 2, None, None]
        ys = rows[:, 3, None, None] * u[None, None, :] + rows[:, 4, None, None] * v[None, :, None] + rows[:, 5, None, None]
        inside = ((xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)).float()
        grid = torch.stack([2 * xs / W - 1, 2 * ys / H - 1], dim=-1)
        zt = z.clone().requires_grad_(True)
        tt = t.clone().requires_grad_(True)

        def torch_loss():
            zt.grad = None
            tw = F.grid_sample(t, grid, mode="bilinear", padding_mode="border", align_corners=False)
            lq = F.log_softmax(tw, dim=1)
            q = lq.exp()
            w = inside * (q.amax(dim=1) >= 0.7).float()
            ((w * (q * (lq - F.log_softmax(zt, dim=1))).sum(dim=1)).sum() / (B * H * W)).backward()

        def torch_adjoint():
            tt.grad = None
            F.grid_sample(tt, grid, mode="bilinear", padding_mode="zeros", align_corners=False).backward(z)

        # the two formulations agree (interior taps are the same rule; the borders differ by the clamp only)
        fused()
        torch_loss()
        # (a pixel whose confidence falls on the other side of tau in the tensor library's float32 softmax differs by a whole
        # gradient: the count of such pixels is given beside the maximum over the rest)
        diff = (dz - zt.grad).abs().amax(dim=1) / zt.grad.abs().max()
        flipped = diff > 1e-3
        agree = diff[~flipped].max().item()
        say(f"(B,C,H,W) = {(B, Cc, H, W)}: fused gradient against the tensor library's float32 formulation: {int(flipped.sum())} of "
            f"{diff.numel()} pixels differ by more than 1e-3 of the largest gradient (decisions at tau), the others by at most {agree:.1e} of it")
        px = B * H * W
        loss_bytes = px * Cc * 4 * 3                    # student in, teacher in (about once), gradient out
        m1 = compare("1. fused loss against the tensor library's ops (forward + backward)",
                     [("wsdl_consistency_fwd_bwd (kl, all, rows)", fused), ("grid_sample + softmax + KL, autograd", torch_loss)], None)
        m2 = compare("2. fused loss against warp_scores_fwd + loss without rows",
                     [("wsdl_consistency_fwd_bwd (kl, all, rows)", fused), ("wsdl_warp_scores_fwd + wsdl_consistency_fwd_bwd", unfused),
                      ("wsdl_consistency_fwd_bwd (kl, counted: three launches)", lambda: fused(1))], loss_bytes)
        m3 = compare("3. fused loss against the cross-entropy kernel",
                     [("wsdl_consistency_fwd_bwd (kl, all, rows)", fused), ("wsdl_softmax_ce_fwd_bwd", ce)], None)
        m4 = compare("4. the adjoint against autograd's backward of grid_sample",
                     [("wsdl_warp_scores_bwd", adjoint), ("grid_sample forward + backward, autograd", torch_adjoint)], None)
        for title, m in (("1", m1), ("2", m2), ("3", m3), ("4", m4)):
            names = list(m)
            verdicts.append(f"{(B, Cc, H, W)} comparison {title}: {names[0]} {'WINS' if m[names[0]] < m[names[1]] else 'LOSES'} "
                            f"against {names[1]} ({m[names[0]]:.1f} us vs {m[names[1]]:.1f} us)")
        del z, t, warped, dsrc, dz, zt, tt, grid, xs, ys, inside
        torch.cuda.empty_cache()
    say("verdicts (comparison 4 times grid_sample's forward too: autograd cannot run its backward alone):")
    for vline in verdicts:
        say("  " + vline)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
