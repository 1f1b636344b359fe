#!/usr/bin/env python3
"""Timing of the score-histogram kernels (csrc/score_hist.hip) at the two segmentation batch shapes, planes (16,256,256) and
(8,512,512), G = 2 groups (int64), 256 bins on [0, 1]; 15 bins for the confidence kernel at C = 2 and 21.

  hist       ``wsdl_score_hist`` through the C ABI (ctypes, no Python checks), counts only and with sums, on three contents: noise,
             a CAM-like plane with 60 % exact zeros, and a flat plane - every pixel in ONE slot, the expected worst case of a
             histogram with LDS atomics, which the wave aggregation is there to hold
  torch      the same contract with the tensor library's ops on the device: ``bucketize`` + ``bincount`` of a combined key
             (asserted equal before timing)
  copy       a ``copy_`` of as many bytes as the histogram reads (12 B/px): the memory yardstick
  sweep      what ``sweep_cam_thresholds`` does after the CAM for 255 thresholds - one histogram + one curve launch - against 255
             calls of thresholding + ``ops.iou_counts``
  otsu       histogram + ``ops.otsu_threshold`` + ``ops.threshold_per_image`` against the fixed-threshold compare they replace
  confidence ``wsdl_confidence_hist`` against ``ops.teacher_targets`` on the same logits (both read every logit twice)
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds after a warm-up, min .. max
beside the mean.  No time or ratio is fixed in advance: the file records what was measured.  The resource report of the kernels
comes from the compiler (``-Rpass-analysis=kernel-resource-usage``).  Writes profiles/score_hist_bench.txt (``--out`` elsewhere)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from weaklysuperviseddl_amd import _build, ops  # noqa: E402
from weaklysuperviseddl_amd._lib import check, lib  # noqa: E402

SHAPES = ((16, 256, 256), (8, 512, 512))
BINS = 256
CONTENTS = ("noise", "cam60", "one_slot")
_KEEP = []          # host arrays whose addresses went into C-ABI calls


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def kernel_resources():
    """[(kernel, VGPRs, SGPRs, LDS, scratch, occupancy)] of csrc/score_hist.hip from the compiler's resource report, or a reason."""
    src = os.path.join(_build.CSRC, "score_hist.hip")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                                                   os.path.join(tmp, "score_hist.o")], capture_output=True, text=True, timeout=300)
    except Exception as exc:        # no compiler where the tool runs
        return f"not measured ({exc})"
    if r.returncode != 0:
        return "not measured (the compile failed)"
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(.*?):? +(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key.startswith("Function Name"):
            demangled = subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip() or val
            cur = {"name": re.sub(r"\(.*", "", demangled.replace("(anonymous namespace)::", "")).replace("void ", "")}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    return [(r_["name"], r_.get("VGPRs", "?"), r_.get("TotalSGPRs", "?"), r_.get("LDS Size [bytes/block]", "?"),
             r_.get("ScratchSize [bytes/lane]", "?"), r_.get("Occupancy [waves/SIMD]", "?")) for r_ in rows]


def plane(content, shape, dev, g):
    if content == "noise":
        return torch.rand(shape, device=dev, generator=g)
    if content == "cam60":
        return torch.where(torch.rand(shape, device=dev, generator=g) < 0.6, torch.zeros((), device=dev), torch.rand(shape, device=dev, generator=g) ** 2)
    return torch.full(shape, 0.5, device=dev)


def hist_variants(shape, content, dev):
    B, H, W = shape
    g = torch.Generator(device=dev).manual_seed(B + H)
    v = plane(content, shape, dev, g)
    grp = (torch.rand(shape, device=dev, generator=g) < 0.4).long()
    if content == "one_slot":
        grp.fill_(1)
    edges = ops.uniform_edges(0.0, 1.0, BINS, dev)
    host = ops.uniform_edges(0.0, 1.0, BINS)
    _KEEP.append(host)
    counts = torch.empty(B, 2, BINS + 3, dtype=torch.int64, device=dev)
    sums = torch.empty_like(counts)
    L, st = lib(), torch.cuda.current_stream(dev).cuda_stream
    args = (v.data_ptr(), grp.data_ptr(), edges.data_ptr(), host.ctypes.data, B, H * W, 2, BINS, 1, counts.data_ptr())
    hist = lambda: check(L.wsdl_score_hist(*args, None, st))  # noqa: E731
    hist_sums = lambda: check(L.wsdl_score_hist(*args, sums.data_ptr(), st))  # noqa: E731
    item = (torch.arange(B, device=dev) * (2 * (BINS + 3))).view(B, 1, 1)

    def torch_fn():
        key = torch.bucketize(v, edges, right=True) + grp * (BINS + 3) + item
        return torch.bincount(key.flatten(), minlength=B * 2 * (BINS + 3)).view(B, 2, BINS + 3)
    a, b = torch.empty(B * H * W * 3, device=dev), torch.empty(B * H * W * 3, device=dev)
    copy = lambda: b.copy_(a)  # noqa: E731
    hist()
    assert torch.equal(counts, torch_fn()), content
    return [("hist", hist), ("hist+sums", hist_sums), ("torch", torch_fn), ("copy", copy)], B * H * W * 12


def sweep_variants(shape, dev):
    B, H, W = shape
    g = torch.Generator(device=dev).manual_seed(7)
    cam = plane("cam60", shape, dev, g)
    gt = (torch.rand(shape, device=dev, generator=g) < 0.4).long()
    th = ops.uniform_edges(0.0, 1.0, 256)[1:]
    edges = torch.from_numpy(th).to(dev)
    out, cv = {}, torch.empty(B, 255, 4, dtype=torch.int64, device=dev)

    def swept():
        return ops.threshold_curves(ops.score_histogram(cam, gt, edges=edges, num_groups=2, out=out), out=cv)

    def one_by_one():
        return [ops.iou_counts((cam >= float(t)).long(), gt, 2, per_image=True) for t in th]
    got, want = swept(), one_by_one()
    for k in (0, 76, 254):          # iou_counts: [..., 0] = intersection, [..., 1] = union of class 1
        assert torch.equal(got[:, k, 0], want[k][:, 1, 0]) and torch.equal(got[:, k, :3].sum(dim=1), want[k][:, 1, 1]), k
    return [("swept", swept), ("255 calls", one_by_one)]


def otsu_variants(shape, dev):
    g = torch.Generator(device=dev).manual_seed(9)
    cam = plane("cam60", shape, dev, g)
    edges = ops.uniform_edges(0.0, 1.0, BINS, dev)
    hout, tout = {}, {}

    def adaptive():
        counts = ops.score_histogram(cam, edges=edges, out=hout)
        return ops.threshold_per_image(cam, ops.otsu_threshold(counts, edges, fallback=0.3)[1], out=tout)
    fixed = lambda: ((cam >= 0.3) & (cam > 0)).to(torch.uint8)  # noqa: E731
    return [("otsu", adaptive), ("fixed", fixed)]


def confidence_variants(shape, C_, dev):
    B, H, W = shape
    g = torch.Generator(device=dev).manual_seed(C_)
    z = torch.randn(B, C_, H, W, device=dev, generator=g) * 3
    y = torch.randint(0, C_, (B, H, W), device=dev, generator=g)
    edges, host = ops.uniform_edges(0.0, 1.0, 15, dev), ops.uniform_edges(0.0, 1.0, 15)
    _KEEP.append(host)
    counts = torch.empty(1, 2, 18, dtype=torch.int64, device=dev)
    sums = torch.empty_like(counts)
    L, st = lib(), torch.cuda.current_stream(dev).cuda_stream
    conf = lambda: check(L.wsdl_confidence_hist(z.data_ptr(), y.data_ptr(), edges.data_ptr(), host.ctypes.data, B, C_, H, W, -100, 15, 0,  # noqa: E731
                                                counts.data_ptr(), sums.data_ptr(), None, None, st))
    tau = torch.full((1,), 0.9, device=dev)
    out = torch.empty_like(y)
    teacher = lambda: check(L.wsdl_teacher_targets(z.data_ptr(), y.data_ptr(), B, C_, H, W, tau.data_ptr(), 0, -100, out.data_ptr(), None, None, st))  # noqa: E731
    return [("confidence_hist", conf), ("teacher_targets", teacher)]


def measure(variants, args, reps=None):
    reps = reps or args.reps
    for _name, fn in variants:
        for _ in range(min(args.warmup, reps)):
            fn()
    rounds = [[time_round(fn, reps) for _name, fn in variants] for _ in range(args.rounds)]
    res = {}
    for i, (name, _fn) in enumerate(variants):
        t = [r[i] for r in rounds]
        res[name] = (sum(t) / len(t), min(t), max(t))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_hist_bench.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_hist_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    fmt = lambda r: f"{r[0]:9.2f} us ({r[1]:9.2f} .. {r[2]:9.2f})"  # noqa: E731
    lines = [f"tools/score_hist_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round after {args.warmup} warm-up "
             f"calls, {args.rounds} rounds, the variants alternating inside a round; us per call = mean (min .. max over the rounds)"]
    res = kernel_resources()
    lines.append("kernel resources of csrc/score_hist.hip (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage); "
                 "score_hist_kernel<V, SUMS, CONF>: V pixels per lane; its LDS is dynamic (table copies + edges, set per launch)")
    if isinstance(res, str):
        lines.append("  " + res)
    else:
        lines.append(f"  {'kernel':44s} VGPRs SGPRs  LDS B scratch B/lane waves/SIMD")
        lines += [f"  {n:44s} {v:>5s} {s:>5s} {l:>6s} {sc:>14s} {o:>10s}" for n, v, s, l, sc, o in res]
    worst = []
    for shape in SHAPES:
        lines.append(f"planes {shape}, groups int64, G = 2, {BINS} bins:")
        base = {}
        for content in CONTENTS:
            variants, nbytes = hist_variants(shape, content, dev)
            r = measure(variants, args)
            base[content] = r
            lines.append(f"  {content}: the histogram reads {nbytes / 1e6:.1f} MB")
            for name, _fn in variants:
                rate = f"  {nbytes / r[name][0] / 1e6:6.3f} TB/s" if name != "torch" else ""
                lines.append(f"    {name:10s} {fmt(r[name])}{rate}")
            lines.append(f"    hist / copy = {r['hist'][0] / r['copy'][0]:.2f}, torch / hist = {r['torch'][0] / r['hist'][0]:.2f}")
        ratio = base["one_slot"]["hist"][0] / base["noise"]["hist"][0]
        ratio_s = base["one_slot"]["hist+sums"][0] / base["noise"]["hist+sums"][0]
        worst.append((shape, ratio, ratio_s, base["cam60"]["hist"][0] / base["noise"]["hist"][0]))
        r = measure(sweep_variants(shape, dev), args, reps=3)
        lines.append(f"  sweep, 255 thresholds: histogram + curves {fmt(r['swept'])}; 255 x (threshold + iou_counts) {fmt(r['255 calls'])}; "
                     f"ratio {r['255 calls'][0] / r['swept'][0]:.1f}")
        r = measure(otsu_variants(shape, dev), args)
        lines.append(f"  per-image Otsu mask (ops.score_histogram + otsu_threshold + threshold_per_image: 3 launches, 1 memset) {fmt(r['otsu'])}; the fixed compare "
                     f"in torch ops {fmt(r['fixed'])}; ratio {r['otsu'][0] / r['fixed'][0]:.2f}")
        for C_ in (2, 21):
            r = measure(confidence_variants(shape, C_, dev), args)
            lines.append(f"  confidence, C = {C_}, 15 bins: wsdl_confidence_hist {fmt(r['confidence_hist'])}; wsdl_teacher_targets "
                         f"{fmt(r['teacher_targets'])}; ratio {r['confidence_hist'][0] / r['teacher_targets'][0]:.2f}")
    held = all(r <= 1.5 and rs <= 1.5 for _s, r, rs, _c in worst)
    is_worst = all(r >= 1.0 and r >= c for _s, r, _rs, c in worst)
    lines.append("expectation: the all-one-slot plane is the worst case of the three contents - " + ("CONFIRMED" if is_worst else "REFUTED")
                 + "; the wave aggregation holds it within 1.5x of noise - " + ("CONFIRMED" if held else "REFUTED") + ": "
                 + "; ".join(f"{s[0]}x{s[1]}x{s[2]} one-slot / noise {r:.2f} (with sums {rs:.2f}), 60 %-zeros / noise {c:.2f}" for s, r, rs, c in worst))
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it (a ctypes call for the C-ABI variants, the Python checks for the ops.* variants).  The "
                 "buffers are reused call after call and the smaller shape fits the last-level cache: the TB/s are algorithmic bytes over "
                 "time, not HBM rates.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
