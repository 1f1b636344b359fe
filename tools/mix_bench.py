#!/usr/bin/env python3
"""Timing of batch mixing (csrc/mix.hip) at the two segmentation batch shapes, images (16,3,256,256) and (8,3,512,512), with what
a mixed teacher step hands over: images, int64 labels, a pixel weight and 2-class scores - 32 B/px read and 32 B/px written,
plus the mask's source (boxes: nothing per pixel; a class set: the partner's int64 label, 8 B/px).

Per shape and for cutmix, classmix and copy_paste:
  apply    the ``ops.mix_batch`` launch alone, outputs preallocated (the selected sets of the class kinds made beforehand)
  call     the whole ``augment.Mix.apply``: for the class kinds the memset, the presence launch and the selection launch in front
  torch    the same contract with the tensor library's ops on the device: the mask from comparisons (boxes) or from a per-image
           ``bincount`` presence table, the splitmix64 keys in wrapped int64 arithmetic and a sort (class sets), no host read;
           then an index by partner and a ``where`` per tensor.  Its results are asserted equal to the device's before timing.
  copy     a ``copy_`` that reads and writes as many bytes as the apply launch: the memory yardstick
Device-event times over back-to-back calls, the variants alternating inside a round, three rounds after a warm-up, min .. max
beside the mean.  No ratio is fixed in advance: the file records what was measured.  The resource report of the kernels comes
from the compiler (``-Rpass-analysis=kernel-resource-usage``).  Writes profiles/mix_bench.txt (``--out`` elsewhere)."""
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
from weaklysuperviseddl_amd.augment import Mix  # noqa: E402

SHAPES = ((16, 3, 256, 256), (8, 3, 512, 512))
C_SCORES = 2
KINDS = ("cutmix", "classmix", "copy_paste")
_M64 = (1 << 64) - 1


def _i64(v):
    """A 64-bit pattern as the int64 of the same bits."""
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def time_round(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def _lsr(z, n):
    return (z >> n) & ((1 << (64 - n)) - 1)


class TorchMix:
    """The contract with the tensor library's own kernels on the device (constants made once); int64 arithmetic wraps modulo
    2^64, logical shifts are masked arithmetic ones, unsigned order is signed order of ``key ^ 2^63``."""

    def __init__(self, B, H, W, C, candidates, dev):
        self.B, self.C = B, C
        self.ys = torch.arange(H, device=dev).view(1, 1, H, 1)
        self.xs = torch.arange(W, device=dev).view(1, 1, 1, W)
        self.item = torch.arange(B, device=dev)
        self.cls = torch.arange(C, device=dev)
        self.step = (self.cls + 1) * _i64(0x9E3779B97F4A7C15)
        cand = torch.zeros(C, dtype=torch.bool, device=dev)
        cand[list(range(C) if candidates is None else candidates)] = True
        self.cand = cand
        self.m1, self.m2, self.sign = _i64(0xBF58476D1CE4E5B9), _i64(0x94D049BB133111EB), _i64(1 << 63)

    def box_mask(self, boxes):
        b = boxes.long()
        y0, x0, y1, x1 = (b[..., k].view(self.B, -1, 1, 1) for k in range(4))
        return ((self.ys >= y0) & (self.ys < y1) & (self.xs >= x0) & (self.xs < x1)).any(dim=1)

    def select(self, labels, seeds):
        B, C = self.B, self.C
        ok = (labels >= 0) & (labels < C)
        flat = (torch.where(ok, labels, torch.zeros_like(labels)) + self.item.view(B, 1, 1) * C).flatten()
        counts = torch.bincount(flat, weights=ok.flatten().to(torch.float32), minlength=B * C).view(B, C)
        present = (counts > 0) & self.cand
        z = seeds.view(B, 1) + self.step
        z = (z ^ _lsr(z, 30)) * self.m1
        z = (z ^ _lsr(z, 27)) * self.m2
        z = z ^ _lsr(z, 31)
        order = z ^ self.sign                                        # unsigned order as signed order
        # rank among the present classes by (key, c): absent classes go behind everything (a stable sort keeps c ascending)
        rank_key = torch.where(present, order, torch.full_like(order, (1 << 63) - 1))
        idx = torch.sort(rank_key, dim=1, stable=True).indices
        k = (present.sum(dim=1, keepdim=True) + 1) // 2
        chosen = torch.zeros_like(present).scatter_(1, idx, self.cls.view(1, C).expand(B, C) < k)
        return chosen & present

    def class_mask(self, labels, sel_table, pb):
        lab = labels[pb]
        ok = (lab >= 0) & (lab < self.C)
        return ok & torch.gather(sel_table[pb], 1, torch.where(ok, lab, torch.zeros_like(lab)).flatten(1)).view_as(lab)

    def __call__(self, kind, tensors, partner, boxes, labels, seeds):
        mixed = (partner >= 0) & (partner < self.B)
        pb = torch.where(mixed, partner.long(), self.item)
        if kind == "cutmix":
            M = self.box_mask(boxes)
        else:
            M = self.class_mask(labels, self.select(labels, seeds), pb)
        M = M & mixed.view(-1, 1, 1)
        return [torch.where(M if t.dim() == 3 else M[:, None], t[pb], t) for t in tensors], M


def kernel_resources():
    """[(kernel, VGPRs, SGPRs, LDS, scratch, occupancy)] of csrc/mix.hip from the compiler's resource report, or a reason."""
    src = os.path.join(_build.CSRC, "mix.hip")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                                                   os.path.join(tmp, "mix.o")], capture_output=True, text=True, timeout=300)
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


def variants_for(shape, kind, dev):
    B, Ci, H, W = shape
    g = torch.Generator(device=dev).manual_seed(B + H)
    img = torch.randn(B, Ci, H, W, device=dev, generator=g)
    lab = (torch.rand(B, H, W, device=dev, generator=g) > 0.5).long()
    lab[:, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
    pw = torch.rand(B, H, W, device=dev, generator=g)
    sc = torch.randn(B, C_SCORES, H, W, device=dev, generator=g)
    mix = Mix(kind, prob=0.9, partner="permute")
    par = Mix.step_params(mix.epoch_params(1, B, (H, W), dev, torch.Generator().manual_seed(1)), 0)
    out = {"images": torch.empty_like(img), "labels": torch.empty_like(lab), "pixel_weight": torch.empty_like(pw), "scores": torch.empty_like(sc)}
    tensors = [img, lab, pw, sc]
    tm = TorchMix(B, H, W, C_SCORES, mix.candidates, dev)
    px = B * H * W
    own = sum(t.element_size() * (t.shape[1] if t.dim() == 4 else 1) for t in tensors)         # B/px read = B/px written
    src = 0 if kind == "cutmix" else 8
    if kind == "cutmix":
        apply = lambda: ops.mix_batch(img, lab, par["partner"], kind="box", boxes=par["boxes"], pixel_weight=pw, scores=sc, out=out)  # noqa: E731
    else:
        sel, _ = ops.mix_class_select(lab, C_SCORES, par["seeds"], candidates=mix.candidates)
        apply = lambda: ops.mix_batch(img, lab, par["partner"], kind="class", class_labels=lab, sel=sel, pixel_weight=pw, scores=sc, out=out)  # noqa: E731
    call = lambda: mix.apply(img, lab, par, num_classes=C_SCORES, pixel_weight=pw, scores=sc, out=out)  # noqa: E731
    torch_fn = lambda: tm(kind, tensors, par["partner"], par["boxes"], lab, par["seeds"])  # noqa: E731
    n_copy = px * (2 * own + src) // 2 // 4                         # floats: read + written = the apply launch's bytes
    a, b = torch.empty(n_copy, device=dev), torch.empty(n_copy, device=dev)
    copy = lambda: b.copy_(a)  # noqa: E731
    # the torch formulation is the same contract: equal results, bit for bit, before anything is timed
    res = mix.apply(img, lab, par, num_classes=C_SCORES, pixel_weight=pw, scores=sc, want_mask=True)
    want, M = torch_fn()
    for got, w in zip((res.images, res.labels, res.pixel_weight, res.scores), want):
        assert torch.equal(got, w), kind
    assert torch.equal(res.mask, M.to(torch.uint8)), kind
    share = float(M.float().mean())
    return [("apply", apply), ("call", call), ("torch", torch_fn), ("copy", copy)], px * (2 * own + src), share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs a GPU (a time measured elsewhere is not a measurement)")
    dev = torch.device("cuda:0")
    lines = [f"tools/mix_bench.py on {torch.cuda.get_device_name(0)}: {args.reps} back-to-back calls per round after {args.warmup} warm-up calls, "
             f"{args.rounds} rounds, the variants alternating inside a round; us per call = mean (min .. max over the rounds)"]
    res = kernel_resources()
    lines.append("kernel resources of csrc/mix.hip (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage); "
                 "mix_apply_kernel<V>: V pixels per lane")
    if isinstance(res, str):
        lines.append("  " + res)
    else:
        lines.append(f"  {'kernel':32s} VGPRs SGPRs  LDS B scratch B/lane waves/SIMD")
        lines += [f"  {n:32s} {v:>5s} {s:>5s} {l:>6s} {sc:>14s} {o:>10s}" for n, v, s, l, sc, o in res]
    notes = []
    for shape in SHAPES:
        lines.append(f"images {shape}, labels int64, pixel weight, scores C = {C_SCORES}:")
        for kind in KINDS:
            variants, nbytes, share = variants_for(shape, kind, dev)
            for _name, fn in variants:
                for _ in range(args.warmup):
                    fn()
            rounds = [[time_round(fn, args.reps) for _name, fn in variants] for _ in range(args.rounds)]
            mean = {}
            launches = ops.mix_launches("box" if kind == "cutmix" else "class", select=kind != "cutmix")
            what = {"apply": "ops.mix_batch, 1 launch", "call": f"Mix.apply, {launches['kernels']} launches + {launches['memsets']} memsets",
                    "torch": "the same contract with torch ops", "copy": "copy_ of the same bytes"}
            lines.append(f"  {kind}: {share * 100:.0f} % of the pixels taken from the partner; the apply launch reads + writes {nbytes / 1e6:.1f} MB")
            for i, (name, _fn) in enumerate(variants):
                t = [r[i] for r in rounds]
                mean[name] = sum(t) / len(t)
                rate = f"  {nbytes / mean[name] / 1e6:6.3f} TB/s" if name in ("apply", "copy") else ""
                lines.append(f"    {name:6s} {what[name]:44s} {mean[name]:9.2f} us ({min(t):9.2f} .. {max(t):9.2f}){rate}")
            spread = max((max(r[i] for r in rounds) - min(r[i] for r in rounds)) / mean[n] for i, (n, _f) in enumerate(variants))
            lines.append(f"    apply / copy = {mean['apply'] / mean['copy']:.2f}, torch / call = {mean['torch'] / mean['call']:.2f}; spread over the "
                         f"rounds up to {spread * 100:.1f} % of a mean")
            notes.append((shape, kind, mean["apply"] / mean["copy"], mean["torch"] / mean["call"]))
    near = all(r <= 1.25 for _s, _k, r, _t in notes)
    below = all(t >= 2.0 for _s, _k, _r, t in notes)
    lines.append("expectation: the apply launch near the copy (within 1.25x) - " + ("CONFIRMED" if near else "REFUTED")
                 + "; the whole call well below the torch formulation (at least 2x) - " + ("CONFIRMED" if below else "REFUTED")
                 + ": " + "; ".join(f"{s[0]}x{s[2]} {k} {r:.2f} / {t:.2f}" for s, k, r, t in notes))
    lines.append("Times are device-event intervals over back-to-back calls on one stream: each includes launch gaps and the host time of the "
                 "call where the device waits for it.  The buffers are reused call after call and the smaller shape fits the last-level "
                 "cache: the TB/s are algorithmic bytes over time, not HBM rates.  A lane whose four pixels all come from one side reads "
                 "that side only, so the bytes counted are the bytes the launch needs.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
