"""ops.augment_batch (csrc/augment.hip) against the launches of the tensor library it replaces in the device loaders; writes
text lines to --out (default profiles/augment_bench.txt) and prints them, then one JSON line.  Every time is taken with
device events after warm-up; the variants of a case alternate inside every round, and the spread over the rounds is printed
beside the mean.

Two cases, both B = 16 items drawn at random from N = 3680 resident ones (64 different index / parameter sets cycled, 0.8 GB
of distinct source items: no set is served from a cache the previous call warmed):
  float   3 x 256 x 256 float32 images + uint8 masks (InMemoryPseudoDataset.batches)
          plain:  images[idx], masks[idx].long()
  uint8   3 x 224 x 224 uint8 images + uint8 trimaps (PetDataset.DeviceLoader)
          plain:  table[images[idx].to(int32)], (trimaps[idx] == 1).long()
and per case ops.augment_batch with the identity rows, and with rows drawn by Augment(scale=(0.5, 2), rotate=30) under
fill="ignore" and fill="reflect".

bytes = the batch's source items once + both outputs once, computed from the shapes (the same count for every variant: a
warp reads at most a few percent more through its clamped taps, a shrinking one less); bytes / time is given as a share of
the achievable HBM rate (--hbm-tbs, 6.3 TB/s measured for an MI355X; the 8 TB/s of the data sheet is not reachable)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, sets, warmup, steps):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(sets[i % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps          # us per batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3680)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a GPU (nothing is measured without one)")
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.augment import Augment
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines, res = [], {"n": a.n, "batch": a.batch, "hbm_tbs": a.hbm_tbs}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/augment_bench.py on {torch.cuda.get_device_name(0)}: B = {a.batch} of N = {a.n}, {a.sets} index sets, "
        f"{a.steps} calls per round, {a.rounds} rounds; us per batch = mean (min .. max over the rounds)")
    for case, side, dtype in (("float", 256, torch.float32), ("uint8", 224, torch.uint8)):
        images = torch.empty(a.n, 3, side, side, dtype=dtype, device=dev)
        for s in range(0, a.n, 256):          # filled in chunks: no second copy of 2.9 GB
            m = min(256, a.n - s)
            if dtype == torch.float32:
                images[s:s + m] = torch.randn(m, 3, side, side, device=dev)
            else:
                images[s:s + m] = torch.randint(0, 256, (m, 3, side, side), device=dev, dtype=torch.uint8)
        if case == "float":
            labels = (torch.rand(a.n, side, side, device=dev) > 0.5).to(torch.uint8) * 255
            lut = label_lut = None

            def plain(s, images=images, labels=labels):
                return images[s[0]], labels[s[0]].long()
        else:
            labels = torch.randint(1, 4, (a.n, side, side), device=dev, dtype=torch.uint8)
            table = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).to(dev)
            lut = table.view(1, 256).repeat(3, 1).contiguous()
            label_lut = torch.zeros(256, dtype=torch.int64, device=dev)
            label_lut[1] = 1

            def plain(s, images=images, labels=labels, table=table):
                return table[images[s[0]].to(torch.int32)], (labels[s[0]] == 1).to(torch.int64)

        warp = Augment(scale=(0.5, 2.0), rotate=30.0)
        ident = Augment.identity()
        sets = []
        for _ in range(a.sets):
            idx = torch.randint(0, a.n, (a.batch,), generator=g).to(dev)
            sets.append((idx, ident.draw(a.batch, (side, side), (side, side)).to(dev),
                         warp.draw(a.batch, (side, side), (side, side), g).to(dev)))

        def fused(which, fill, images=images, labels=labels, lut=lut, label_lut=label_lut):
            return lambda s: ops.augment_batch(images, labels, s[0], s[which], lut=lut, label_lut=label_lut, fill=fill)

        variants = [("plain torch launches", plain), ("augment_batch identity", fused(1, "ignore")),
                    ("augment_batch warp, ignore", fused(2, "ignore")), ("augment_batch warp, reflect", fused(2, "reflect"))]
        # the identity is what the loaders promise: check it here too, at the size that is timed
        want, got = plain(sets[0]), variants[1][1](sets[0])
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        px = a.batch * side * side
        nbytes = px * 3 * images.element_size() + px + px * 3 * 4 + px * 8
        times = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                times[name].append(timed(fn, sets, a.warmup, a.steps))
        say(f"{case}: 3 x {side} x {side} {str(dtype).replace('torch.', '')} source; {nbytes / 1e6:.2f} MB per batch "
            f"(source items + outputs, once each)")
        base = sum(times[variants[0][0]]) / a.rounds
        for name, _ in variants:
            t = times[name]
            mean = sum(t) / len(t)
            share = nbytes / (mean * 1e-6) / (a.hbm_tbs * 1e12)
            say(f"  {name:28s} {mean:8.2f} us ({min(t):.2f} .. {max(t):.2f})  {nbytes / mean / 1e6:6.2f} TB/s = "
                f"{100 * share:5.1f} % of {a.hbm_tbs:g} TB/s   x{mean / base:.2f} of plain")
            res[f"{case}/{name}"] = {"us": round(mean, 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                     "hbm_share": round(share, 4), "ratio_to_plain": round(mean / base, 3)}
        del images, labels, sets, variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
