#!/usr/bin/env python3
"""Timing of the EMA teacher's launches (csrc/ema.hip) at the real size: the flat buffer of the DeepLab model (39.6 M parameters, 42.0 M floats
with the padding between them).

  flat      wsdl_flat_ema (12 bytes per element) beside the default Adam launch (wsdl_adam_step_dev, 28 bytes per element) and
            wsdl_flat_step_dev(AdamW) on the same buffers, in one process, the three alternating inside a round
  table     wsdl_ema_table over the model's real float buffers (the BatchNorm running statistics), both modes
  targets   wsdl_teacher_targets at (16,2,256,256), (8,2,512,512) and (8,21,512,512) beside the same contract written with torch
            ops in float32 on the device and beside ops.cross_entropy (forward) on the same bytes
  step      a planned train_step (B = 4, 256 x 256) with an EMA attached beside one without, in one process, alternating
The new kernels and the two step launches are called straight through the C ABI (ctypes, no wrapper in the loop); the
tensor-library formulation and ops.cross_entropy through their Python entry points.  Device-event times over back-to-back calls (200 per round for the kernels, 500 for the table, 40 for the step), three rounds,
min .. max beside the mean; rates are the algorithm's bytes over that time, inside a loop that leaves the Infinity Cache warm.
One derived condition: the EMA launch moves 12 / 28 of the Adam launch's bytes, so an EMA launch slower than the Adam launch is a
defect (the tool says so and exits with status 1).  Registers, LDS and scratch of the kernels as the compiler reports them: ``--resources-only`` prints that
section alone (needs hipcc), ``--no-resources`` leaves it out.  Writes profiles/ema_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

TARGET_SHAPES = ((16, 2, 256, 256), (8, 2, 512, 512), (8, 21, 512, 512))


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3          # microseconds


def alternate(variants, reps, rounds=3, warm=3):
    """{name: [us per round]} with the variants alternating inside each round."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(time_round(fn, reps))
    return out


def fmt(name, ts, nbytes=None):
    mean = sum(ts) / len(ts)
    line = f"  {name:<44s} {mean:10.1f} us   ({min(ts):.1f} .. {max(ts):.1f})"
    if nbytes:
        line += f"   {nbytes / mean / 1e6:7.2f} TB/s"
    return line


def torch_targets(logits, labels, tau, ignore_index=-100):
    p, t = torch.softmax(logits, dim=1).max(dim=1)
    finite = torch.isfinite(logits).all(dim=1)
    ign = labels == ignore_index
    flip = finite & (p >= tau) & (t != labels) & ~ign
    out = torch.where(flip, t, labels)
    conf = torch.where(ign | ~finite, torch.zeros_like(p), p)
    counts = torch.stack([(~flip & ~ign).sum(), flip.sum(), ign.sum()])
    return out, conf, counts


def resources():
    src = os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "ema.hip")
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        return ["  (hipcc not found: no resource report)"]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                            "-o", os.path.join(tmp, "ema.o")], capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": re.sub(r"\(anonymous namespace\)::|\(.*$", "", name)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    return [f"  {r_['name']:<44s} VGPRs {r_.get('VGPRs', '?'):>3s}  SGPRs {r_.get('TotalSGPRs', '?'):>3s}  LDS {r_.get('LDS', '?'):>3s} B  "
            f"scratch {r_.get('ScratchSize', '?')} B/lane  occupancy {r_.get('Occupancy', '?')} waves/SIMD" for r_ in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.txt"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if args.resources_only:
        print("\n".join(["kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):"] + resources()))
        return 0
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd._lib import lib
    from weaklysuperviseddl_amd.ema import FlatEMA
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = [f"tools/ema_bench.py on {torch.cuda.get_device_name(0)}", ""]
    bad = False

    model = build_segmentation_model().to(dev).train()
    opt = make_optimizer(model, lr=1e-4)
    avg = FlatEMA(opt, model, build_segmentation_model().to(dev))
    n = opt.numel
    opt.flat_grad.normal_(0, 1e-3)
    opt.sync_hyper()
    ops.add_int(opt.step_dev, 1)
    # straight through the C ABI (the bound functions of _lib.py): no host-side validation of the Python wrappers in the loop
    L, stream = lib(), ops.raw_stream(dev)
    P = lambda t: t.data_ptr()      # noqa: E731
    pp, gg, mm, vv, ee = (P(t) for t in (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, avg.ema_param))
    hy, he, sd, s0 = P(opt.hyper_dev), P(avg.hyper_dev), P(opt.step_dev), P(avg.start_dev)

    def checked(rc):
        assert rc == 0, L.wsdl_last_error()
    variants = {
        "flat_ema": lambda: checked(L.wsdl_flat_ema(ee, pp, n, he, sd, s0, None, stream)),
        "adam (default launch)": lambda: checked(L.wsdl_adam_step_dev(pp, gg, mm, vv, n, hy, sd, stream)),
        "flat_step_dev(AdamW)": lambda: checked(L.wsdl_flat_step_dev(ops.FLAT_ADAMW, pp, gg, mm, vv, n, None, hy, sd, None, stream)),
    }
    res = alternate(variants, reps=200)
    lines.append(f"flat buffer: {n} floats ({n * 4 / 1e6:.1f} MB)")
    lines.append(fmt("flat_ema", res["flat_ema"], 12 * n))
    lines.append(fmt("adam (default launch)", res["adam (default launch)"], 28 * n))
    lines.append(fmt("flat_step_dev(AdamW)", res["flat_step_dev(AdamW)"], 28 * n))
    ema_us, adam_us = (sum(res[k]) / 3 for k in ("flat_ema", "adam (default launch)"))
    if ema_us > adam_us:
        bad = True
        lines.append("  DEFECT: the EMA launch is slower than the Adam launch although it moves 12 / 28 of its bytes")
    floats = sum(tb.numel() for tb, _ in avg._float_bufs)
    lines += ["", f"buffer table: {len(avg._float_bufs)} tensors, {floats} floats"]
    for mode in ("ema", "copy"):
        code = {"ema": 0, "copy": 1}[mode]
        ts = alternate({mode: lambda: checked(L.wsdl_ema_table(P(avg._table), len(avg._float_bufs), he, sd, s0, None, code, stream))},
                       reps=500)[mode]
        lines.append(fmt(f"ema_table mode {mode}", ts))
    table_us = sum(ts) / len(ts)

    lines += ["", "teacher_targets (tau 0.9, replace, with conf and counts)"]
    for shape in TARGET_SHAPES:
        B, C, H, W = shape
        logits = torch.randn(shape, device=dev) * 3
        labels = torch.randint(0, C, (B, H, W), device=dev)
        labels[torch.rand(B, H, W, device=dev) < 0.1] = -100
        tau = torch.full((1,), 0.9, device=dev)
        out, conf, counts = torch.empty_like(labels), torch.empty(B, H, W, device=dev), torch.zeros(3, device=dev, dtype=torch.int64)
        res = alternate({
            "hip": lambda: checked(L.wsdl_teacher_targets(P(logits), P(labels), B, C, H, W, P(tau), 0, -100, P(out), P(conf), P(counts), stream)),
            "torch": lambda: torch_targets(logits, labels, 0.9),
            "ce": lambda: ops.cross_entropy(logits, labels),
        }, reps=200)
        nbytes = logits.numel() * 4 + labels.numel() * (8 + 8 + 4)
        lines.append(f" {shape}")
        lines.append(fmt("wsdl_teacher_targets", res["hip"], nbytes))
        lines.append(fmt("torch ops, float32", res["torch"]))
        lines.append(fmt("ops.cross_entropy (forward)", res["ce"]))
    del model, opt, avg
    torch.cuda.empty_cache()

    if not args.no_step:
        lines += ["", "planned train_step, B = 4, 256 x 256 (mean of 40 replays per round)"]
        x = torch.randn(4, 3, 256, 256, device=dev)
        m = (torch.rand(4, 256, 256, device=dev) > 0.5).long()
        steps = {}
        for name in ("without EMA", "with EMA"):
            torch.manual_seed(0)
            net = build_segmentation_model().to(dev).train()
            o = make_optimizer(net, lr=1e-4)
            if name == "with EMA":
                FlatEMA(o, net, build_segmentation_model().to(dev))
            for _ in range(4):
                train_step(net, o, x, m)
            st = next(iter(o.__dict__["_wsdl_planned"].values()))
            assert st.disabled is None and st.replays >= 1, st.disabled
            steps[name] = (lambda net=net, o=o: train_step(net, o, x, m))
        res = alternate(steps, reps=40)
        for name in steps:
            lines.append(fmt(name, res[name]))
        diff = sum(res["with EMA"]) / 3 - sum(res["without EMA"]) / 3
        lines.append(f"  difference {diff:.1f} us; expected: flat_ema {ema_us:.1f} us + ema_table {table_us:.1f} us = {ema_us + table_us:.1f} us")
    if not args.no_resources:
        lines += ["", "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):"] + resources()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
