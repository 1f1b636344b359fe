#!/usr/bin/env python3
"""Timing of the flat optimiser's launches at the segmentation model's 39.6 M parameters: the default Adam launch
(adam_kernel, untouched), each algorithm of the flat step kernel (csrc/flat_optim.hip) with and without a weight-decay table,
and the two launches of the gradient norm.  Prints microseconds, bytes per parameter and TB/s against the algorithmic bytes;
three rounds each, alternating the variants inside a round, the spread over the rounds beside every mean.  Writes
profiles/flat_optim_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from weaklysuperviseddl_amd import ops  # noqa: E402

N = 39_633_986 // 64 * 64 + 64      # the flat buffer of the segmentation model, on the 64-float grid
PEAK_TBS = 6.3                       # the figure the other profiles of this directory use


def time_round(fn, reps):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_optim_bench.txt"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flat_optim_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(N, device=dev, generator=g)
    grad = torch.randn(N, device=dev, generator=g) * 1e-3
    m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    step_dev = torch.ones(1, dtype=torch.int32, device=dev)
    stats = torch.tensor([0., 1., 1., 0.], device=dev)
    partials = torch.zeros(ops.grad_norm_partials(), dtype=torch.float64, device=dev)
    # one entry in eight without decay, as BatchNorm parameters and biases lie between the convolution weights
    table = (torch.arange(N // 64, device=dev) % 8 != 3).to(torch.uint8)
    # lr, beta1, beta2, eps, grad_scale, weight_decay, momentum, nesterov, max_norm, skip_nonfinite
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1.0, 1e-4, 0.9, 0.0, 1.0, 1.0], device=dev)

    lib, P, S = ops.lib(), ops._p, ops._stream
    variants = [
        ("adam (default launch, adam_kernel)", 28, lambda: ops.adam_step_flat(p, grad, m, v, 0, 0, 0, 0, 0, step_dev=step_dev, hyper_dev=hyper)),
        ("adam + L2, no table", 28, lambda: ops.flat_step(ops.FLAT_ADAM_L2, p, grad, m, v, hyper, step_dev)),
        ("adamw, no table", 28, lambda: ops.flat_step(ops.FLAT_ADAMW, p, grad, m, v, hyper, step_dev)),
        ("adamw, table", 28 + 1 / 64, lambda: ops.flat_step(ops.FLAT_ADAMW, p, grad, m, v, hyper, step_dev, None, table)),
        ("adamw, table, clip + skip (stats_dev)", 28 + 1 / 64, lambda: ops.flat_step(ops.FLAT_ADAMW, p, grad, m, v, hyper, step_dev, stats, table)),
        ("sgd momentum, table", 20 + 1 / 64, lambda: ops.flat_step(ops.FLAT_SGD, p, grad, m, None, hyper, step_dev, None, table)),
        ("sgd without momentum (m = NULL)", 12, lambda: ops.flat_step(ops.FLAT_SGD, p, grad, None, None, hyper, step_dev)),
        ("norm: squares -> partials", 4, lambda: ops.check(lib.wsdl_grad_sqnorm_partials(P(grad), N, P(partials), S()))),
        ("norm: finalize (1 workgroup)", 0, lambda: ops.check(lib.wsdl_grad_clip_finalize(P(partials), partials.numel(), P(hyper), P(step_dev), P(stats), S()))),
        ("norm: both launches (ops.grad_norm)", 4, lambda: ops.grad_norm(grad, hyper, step_dev, stats, partials)),
    ]
    for _name, _b, fn in variants:          # warm up every variant: code objects load at the first launch
        for _ in range(5):
            fn()
    rounds = [[time_round(fn, args.reps) for _name, _b, fn in variants] for _ in range(args.rounds)]

    lines = [f"tools/flat_optim_bench.py on {torch.cuda.get_device_name(0)}: {N} parameters ({4 * N / 1e6:.1f} MB per buffer), {args.reps} "
             f"back-to-back launches per round, {args.rounds} rounds, the variants alternating inside a round; us = mean (min .. max over the rounds)"]
    means = []
    for i, (name, bpp, _fn) in enumerate(variants):
        t = [r[i] for r in rounds]
        mean = sum(t) / len(t)
        means.append(mean)
        rate = f"{bpp * N / mean / 1e6:6.2f} TB/s = {bpp * N / mean / 1e6 / PEAK_TBS * 100:5.1f} % of {PEAK_TBS} TB/s" if bpp else " " * 33
        lines.append(f"  {name:42s} {mean:9.2f} us ({min(t):9.2f} .. {max(t):9.2f})  {bpp:7.3f} B/param  {rate}  x{mean / means[0]:.3f} of adam")
    spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / means[i] for i in range(7))
    lines.append(f"Run-to-run spread of the step launches over the rounds: up to {spread * 100:.2f} % of the mean.")
    lines.append(f"adamw with a table against the default Adam launch: {(means[3] / means[0] - 1) * 100:+.2f} %; sgd momentum / adam = "
                 f"{means[5] / means[0]:.3f} (bytes: {20 / 28:.3f}); the norm adds {means[9]:.1f} us to a clipped step "
                 f"({means[9] / means[0] * 100:.1f} % of the Adam launch; bytes: {4 / 28 * 100:.1f} %).")
    over = means[3] / means[0] - 1
    if over > spread:
        lines.append(f"Gate (adamw launch against the Adam launch, which this commit does not touch): slower by {over * 100:.2f} % = "
                     f"{means[3] - means[0]:.2f} us, beyond the spread.  Both move 28 B/parameter; what adamw adds is one multiply per "
                     "element, a table byte per 16 lanes and five more scalar loads before the loop - which of them costs the time "
                     "was not separated.")
    else:
        lines.append(f"Gate (adamw launch against the Adam launch, which this commit does not touch): {over * 100:+.2f} %, within the spread.")
    lines.append("Times are device-event intervals over back-to-back launches on one stream: each includes the gap to the next launch.  "
                 "The finalize launch is one workgroup: its time is launch latency.  The same buffers are reused launch after launch, so "
                 "the small working sets (sgd without momentum, the norm) are partly served by the last-level cache: their TB/s are "
                 "not HBM rates.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
