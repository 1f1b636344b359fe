#!/usr/bin/env python3
"""Timing of the signed-distance boundary loss and the surface-distance statistics (csrc/boundary_loss.hip) at the two
segmentation batch shapes, logits (16,2,256,256) and (8,2,512,512), K = 1 class.  No ratio is fixed in advance; everything
below is measured in the same run, the variants alternating inside a round.

  kernel       wsdl_boundary_loss_fwd_bwd against wsdl_softmax_ce_ex_fwd_bwd with a pixel weight in place, both called
               straight through the C ABI (two launches each: the fused pass and its finalize).  Algorithmic bytes per pixel:
               boundary loss 4C (logits) + 4K (phi) + 8 (labels) + 4C (dlogits); cross entropy 4C + 8 + 4 (pixel weight) + 4C -
               the same to within one plane.  The boundary loss evaluates its softmax in double.
  criterion    wnn.CrossEntropyBoundaryLoss forward + backward (phi rebuilt from the labels on every call) against
               wnn.CrossEntropyLoss forward + backward: the cost of the term
  torch        the same contract written with the tensor library's kernels on the device, phi GIVEN: F.cross_entropy + alpha *
               (softmax(logits)[:, 1] * phi).mean(), forward + backward; beside it the library with phi given
               (ops.cross_entropy + ops.boundary_loss(scale=), ops.fanout / ops.add_scalars)
  phi          ops.signed_distance_classes alone (two edt launches and the conversion per class)
  surface      ops.surface_distance_stats (four transforms, the surface map, the statistics, two k-th values) - and, one round
               on the host clock, the call plus its copy to the host against the scipy formulation on the host (binary_erosion,
               distance_transform_edt of the other surface, max / mean / percentile), the copy of the masks included
Device-event times over back-to-back calls, three rounds, min .. max beside the mean.  Writes profiles/boundary_loss_bench.txt
(``--out`` elsewhere)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from weaklysuperviseddl_amd import ops, nn as wnn  # noqa: E402
from weaklysuperviseddl_amd._lib import lib  # noqa: E402

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


def blobs(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        for _ in range(5):
            cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            r = int(torch.randint(H // 16, H // 4, (1,), generator=g))
            out[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return out.to(dev)


def scipy_surface_metrics(ndi, preds, labels, percentile):
    """medpy's surfaces and the directed distances with scipy on the host: [(hd, hd95 (nearest rank), assd (pooled))]."""
    out = []
    for p, g in zip(preds, labels):
        sp, sg = p ^ ndi.binary_erosion(p, border_value=0), g ^ ndi.binary_erosion(g, border_value=0)
        if not sp.any() or not sg.any():
            out.append((float("nan"),) * 3)
            continue
        d = [ndi.distance_transform_edt(~sg)[sp], ndi.distance_transform_edt(~sp)[sg]]
        pct = [np.sort(x)[::-1][min(len(x), 1 + int(np.floor((1.0 - percentile / 100.0) * len(x)))) - 1] for x in d]
        out.append((max(d[0].max(), d[1].max()), max(pct), (d[0].sum() + d[1].sum()) / (len(d[0]) + len(d[1]))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_loss_bench.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_loss_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    L = lib()
    lines = [f"tools/boundary_loss_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round, {args.rounds} "
             "rounds, the variants alternating inside a round; us = mean (min .. max over the rounds); GB/s = algorithmic bytes over the time"]
    for B, Cc, H, W in SHAPES:
        n = B * H * W
        masks = blobs(B, H, W, dev)
        preds = torch.roll(masks, (3, -2), (1, 2)).contiguous()
        logits = torch.randn(B, Cc, H, W, device=dev, requires_grad=True)
        phi = ops.signed_distance_classes(masks, (1,))
        pw = ops.boundary_confidence(masks, 3.0, 0.1)
        alpha = torch.tensor([0.01], device=dev)
        # ---- the two fused kernels through the C ABI
        raw = logits.detach()
        dl, loss, inv = torch.empty_like(raw), torch.empty((), device=dev), torch.empty(1, device=dev)
        ws = ops.workspace(L.wsdl_reduce_workspace(), dev)
        cls = (C.c_int * 1)(1)
        stream = ops.raw_stream(dev)

        def k_boundary():
            ops.check(L.wsdl_boundary_loss_fwd_bwd(raw.data_ptr(), phi.data_ptr(), masks.data_ptr(), cls, 1, loss.data_ptr(), dl.data_ptr(),
                                                   inv.data_ptr(), alpha.data_ptr(), B, Cc, H, W, -100, ws.data_ptr(), ws.numel(), stream))

        def k_ce():
            ops.check(L.wsdl_softmax_ce_ex_fwd_bwd(raw.data_ptr(), masks.data_ptr(), loss.data_ptr(), dl.data_ptr(), inv.data_ptr(), B, Cc, H,
                                                   W, 1.0, -100, None, pw.data_ptr(), 0.0, 0, ws.data_ptr(), ws.numel(), stream))
        bytes_bl, bytes_ce = n * (4 * Cc + 4 + 8 + 4 * Cc), n * (4 * Cc + 8 + 4 + 4 * Cc)
        # ---- criteria
        both = wnn.CrossEntropyBoundaryLoss(alpha=0.01).to(dev)
        plain = wnn.CrossEntropyLoss()

        def fwd_bwd(crit):
            logits.grad = None
            crit(logits, masks).backward()

        def torch_given():
            logits.grad = None
            (F.cross_entropy(logits, masks) + alpha[0] * (torch.softmax(logits, dim=1)[:, 1] * phi[:, 0]).mean()).backward()

        def lib_given():
            logits.grad = None
            a, b = ops.fanout(logits, 2)
            ops.add_scalars(ops.cross_entropy(a, masks), ops.boundary_loss(b, phi, masks, scale=alpha)).backward()
        bufs_phi, bufs_st = {}, {}
        variants = [
            ("kernel: wsdl_boundary_loss_fwd_bwd (C ABI, fused pass + finalize)", bytes_bl, k_boundary),
            ("kernel: wsdl_softmax_ce_ex_fwd_bwd with a pixel weight (C ABI, fused pass + finalize)", bytes_ce, k_ce),
            ("criterion: wnn.CrossEntropyBoundaryLoss forward + backward (phi from the labels)", 0, lambda: fwd_bwd(both)),
            ("criterion: wnn.CrossEntropyLoss forward + backward", 0, lambda: fwd_bwd(plain)),
            ("torch: F.cross_entropy + alpha * mean(softmax * phi), phi given, forward + backward", 0, torch_given),
            ("library: ops.cross_entropy + ops.boundary_loss(scale=), phi given, forward + backward", 0, lib_given),
            ("phi: ops.signed_distance_classes(labels, (1,))", 0, lambda: ops.signed_distance_classes(masks, (1,), out=bufs_phi)),
            ("surface: ops.surface_distance_stats", 0, lambda: ops.surface_distance_stats(preds, masks, out=bufs_st)),
        ]
        lib_given()
        g_lib = logits.grad.clone()
        torch_given()
        agree = ((logits.grad - g_lib).abs().max() / g_lib.abs().max()).item()
        for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
            for _ in range(3):
                fn()
        rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]
        lines.append(f"logits ({B},{Cc},{H},{W}), K = 1, {n} pixels; boundary loss {bytes_bl / 1e6:.1f} MB, cross entropy {bytes_ce / 1e6:.1f} MB "
                     f"algorithmic; max |torch gradient - library gradient| / max |gradient| = {agree:.1e}:")
        means, spreads = [], []
        for i, (name, nbytes, _fn) in enumerate(variants):
            t = [r[i] for r in rounds]
            mean = sum(t) / len(t)
            means.append(mean)
            spreads.append(max(t) - min(t))
            rate = f"{nbytes / mean / 1e3:8.1f} GB/s" if nbytes else ""
            lines.append(f"  {name:92s} {mean:10.2f} us ({min(t):10.2f} .. {max(t):10.2f})  {rate}")
        scaled = means[1] * bytes_bl / bytes_ce
        lines.append(f"  the boundary-loss kernel takes {means[0] / means[1]:.2f}x of the cross-entropy kernel ({means[0] - scaled:+.2f} us against its "
                     f"time scaled by the byte ratio {bytes_bl / bytes_ce:.3f}; run-to-run spreads {spreads[0]:.2f} and {spreads[1]:.2f} us); the "
                     f"criterion takes {means[2] / means[3]:.2f}x of wnn.CrossEntropyLoss (+{means[2] - means[3]:.1f} us, of which "
                     f"{means[6]:.1f} us are the signed distance map); with phi given the torch formulation takes {means[4] / means[5]:.2f}x "
                     "of the library's")
        if ndi is not None:
            ops.surface_distances(preds, masks)          # (the tensor library's kernels of the packing load at the first call)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.surface_distances(preds, masks)
            t_dev = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            want = scipy_surface_metrics(ndi, (preds.cpu() == 1).numpy(), (masks.cpu() == 1).numpy(), 95.0)
            t_host = (time.perf_counter() - t0) * 1e6
            ok = all(abs(p[k] - w[i]) <= 1e-9 * max(1.0, w[i]) for p, w in zip(got[0], want) for i, k in enumerate(("hd", "hd95", "assd")))
            lines.append(f"  scipy (one round, host clock): ops.surface_distances, its one copy to the host included, {t_dev:.0f} us; the scipy "
                         f"formulation per image on the host, the copy of the masks included, {t_host:.0f} us ({t_host / t_dev:.0f}x); equal: {ok}")
        else:
            lines.append("  scipy: not importable here - not measured")
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
