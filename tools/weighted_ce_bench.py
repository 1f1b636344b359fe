"""The fused cross-entropy call (csrc/resample_loss.hip) with and without its options; writes text lines to --out (default
profiles/weighted_ce_bench.txt) and prints them, then one JSON line.

What is timed: the C ABI call itself - wsdl_softmax_ce_fwd_bwd for the default row, wsdl_softmax_ce_ex_fwd_bwd for the
others - with loss AND gradient, i.e. the cross-entropy kernel plus the one-block finalize kernel (no finalize for
reduction 'none'), enqueued back to back on preallocated buffers.  Device events around windows of at least --window seconds
after a warm-up of every buffer set; the buffer sets of a shape are cycled and together exceed --distinct-gb, so that no
call is served from the 256 MiB last-level cache the previous call filled.

bytes = what the algorithm has to move, from the shapes: C planes read + C planes written + 8-byte labels per pixel, + 4
for pixel weights, + 4 for the per-pixel map.  bytes / time is given as a share of the HBM rate (--hbm-tbs: 6.29 TB/s
measured for an MI355X by a float4 copy; the 8 TB/s of the data sheet is not reachable).  It is the share of the whole
call, finalize kernel and launch gaps included, not of the kernel alone.

--parent-lib SO: an A/B of the default call against another build of the library (the parent commit's), both loaded into
this process and alternated; the spread between windows of the SAME build is measured first and is the margin.  The same
option compares loss, gradient and inverse count of the default call, bit for bit, on seeded inputs at every shape."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(16, 2, 256, 256), (8, 2, 512, 512), (16, 3, 256, 256), (16, 21, 256, 256)]
# name -> (class weights, smoothing, pixel weights, reduction)
VARIANTS = [("default", (False, 0.0, False, 0)), ("weight", (True, 0.0, False, 0)), ("smoothing", (False, 0.1, False, 0)),
            ("pixel_weight", (False, 0.0, True, 0)), ("sum", (False, 0.0, False, 1)), ("none", (False, 0.0, False, 2)),
            ("all+mean", (True, 0.1, True, 0)), ("all+none", (True, 0.1, True, 2))]


def algorithm_bytes(shape, pixel, per_pixel_map):
    B, Cc, H, W = shape
    return B * H * W * (8 * Cc + 8 + (4 if pixel else 0) + (4 if per_pixel_map else 0))


class Buffers:
    def __init__(self, shape, dev, seed):
        B, Cc, H, W = shape
        g = torch.Generator().manual_seed(seed)
        self.logits = (torch.randn(shape, generator=g) * 3).to(dev)
        y = torch.randint(0, Cc, (B, H, W), generator=g)
        y[torch.rand(B, H, W, generator=g) < 0.2] = -100
        self.labels = y.to(dev)
        self.pw = torch.rand(B, H, W, generator=g).to(dev)
        self.dl = torch.empty_like(self.logits)
        self.map = torch.empty(B, H, W, device=dev)
        self.loss = torch.empty((), device=dev)
        self.inv = torch.empty(1, device=dev)


def old_call(handle, shape, b, ws, stream):
    B, Cc, H, W = shape
    return lambda: handle.wsdl_softmax_ce_fwd_bwd(b.logits.data_ptr(), b.labels.data_ptr(), b.loss.data_ptr(), b.dl.data_ptr(),
                                                  b.inv.data_ptr(), B, Cc, H, W, 1.0, -100, ws.data_ptr(), ws.numel(), stream)


def ex_call(handle, shape, b, cw, variant, ws, stream):
    B, Cc, H, W = shape
    weighted, eps, pixel, reduction = variant
    out = b.map if reduction == 2 else b.loss
    return lambda: handle.wsdl_softmax_ce_ex_fwd_bwd(b.logits.data_ptr(), b.labels.data_ptr(), out.data_ptr(), b.dl.data_ptr(),
                                                     b.inv.data_ptr(), B, Cc, H, W, 1.0, -100,
                                                     cw.data_ptr() if weighted else None, b.pw.data_ptr() if pixel else None,
                                                     eps, reduction, ws.data_ptr(), ws.numel(), stream)


def window(calls, steps):
    """us per call over one timed window of `steps` calls cycling through `calls`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = len(calls)
    e0.record()
    for i in range(steps):
        if calls[i % n]() != 0:
            raise RuntimeError("the library refused the call")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def steps_for(calls, seconds):
    for c in calls:                 # warm every buffer set
        c()
    torch.cuda.synchronize()
    us = window(calls, 200)
    return max(200, int(math.ceil(seconds * 1e6 / us)))


def load_parent(path):
    h = C.CDLL(path)
    vp, i, ll, f, sz = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t
    h.wsdl_softmax_ce_fwd_bwd.restype = i
    h.wsdl_softmax_ce_fwd_bwd.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, f, ll, vp, sz, vp]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--distinct-gb", type=float, default=0.6)
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_ce_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weighted_ce_bench: needs a GPU (nothing is measured without one)")
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd._lib import lib
    dev = torch.device("cuda:0")
    cur, stream = lib(), ops._stream()
    ws = ops.workspace(cur.wsdl_reduce_workspace(), dev)
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    lines, result = [], {"rows": [], "ab": [], "bit_identical": None}

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"# fused cross entropy, loss + gradient per call; device events, windows of >= {a.window} s, {a.rounds} rounds; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"# share = bytes / time / {a.hbm_tbs} TB/s (achievable HBM rate); buffer sets cycled: > {a.distinct_gb} GB distinct per shape")
    say(f"{'shape':<18}{'variant':<14}{'us/call':>9}{'spread':>8}{'MB':>8}{'GB/s':>8}{'share':>7}{'vs default':>11}{'bytes vs default':>17}")
    sets = {}
    for shape in SHAPES:
        nsets = min(64, max(2, int(math.ceil(a.distinct_gb * 1e9 / algorithm_bytes(shape, True, True)))))
        bufs = sets[shape] = [Buffers(shape, dev, 17 + k) for k in range(nsets)]
        cw = (torch.rand(shape[1], generator=torch.Generator().manual_seed(1)) + 0.25).to(dev)
        base_us = base_bytes = None
        for name, variant in VARIANTS:
            calls = [old_call(cur, shape, b, ws, stream) if name == "default" else ex_call(cur, shape, b, cw, variant, ws, stream)
                     for b in bufs]
            steps = steps_for(calls, a.window)
            us = [window(calls, steps) for _ in range(a.rounds)]
            mean, nbytes = sum(us) / len(us), algorithm_bytes(shape, variant[2], variant[3] == 2)
            if name == "default":
                base_us, base_bytes = mean, nbytes
            gbs = nbytes / mean * 1e-3
            say(f"{'x'.join(map(str, shape)):<18}{name:<14}{mean:9.2f}{(max(us) - min(us)) / mean:8.1%}{nbytes / 1e6:8.1f}{gbs:8.0f}"
                f"{gbs / (a.hbm_tbs * 1e3):7.1%}{mean / base_us:10.3f}x{nbytes / base_bytes:16.3f}x")
            result["rows"].append({"shape": shape, "variant": name, "us": mean, "bytes": nbytes, "gbs": gbs, "steps": steps})
        say()

    if parent is not None:
        say(f"# default call, this build (A) against the parent commit's build (B): {a.ab_rounds} alternating rounds of one window each; "
            "first two windows of A alone")
        say("# margin = the larger of the A-A spread of the first two windows and the spread of A over the rounds")
        say(f"{'shape':<18}{'A us':>9}{'B us':>9}{'A/B':>8}{'A-A spread':>12}{'margin':>8}  verdict")
        worst = 0.0
        for shape in SHAPES:
            bufs = sets[shape]
            ca = [old_call(cur, shape, b, ws, stream) for b in bufs]
            cb = [old_call(parent, shape, b, ws, stream) for b in bufs]
            steps = max(steps_for(ca, a.window), steps_for(cb, a.window))
            a0, a1 = window(ca, steps), window(ca, steps)
            ta, tb = [], []
            for _ in range(a.ab_rounds):
                ta.append(window(ca, steps))
                tb.append(window(cb, steps))
            ma, mb = sum(ta) / len(ta), sum(tb) / len(tb)
            same = abs(a0 - a1) / min(a0, a1)
            margin = max(same, (max(ta) - min(ta)) / ma)
            slower = ma / mb - 1.0
            worst = max(worst, slower - margin)
            verdict = "not slower" if slower <= margin else "SLOWER than the parent beyond the margin"
            say(f"{'x'.join(map(str, shape)):<18}{ma:9.2f}{mb:9.2f}{ma / mb:8.3f}{same:12.1%}{margin:8.1%}  {verdict}")
            result["ab"].append({"shape": shape, "a_us": ma, "b_us": mb, "same_build_spread": same, "margin": margin})
        say()
        same_bits = True
        for shape in SHAPES:
            b = sets[shape][0]
            got = []
            for handle in (cur, parent):
                b.dl.fill_(-7.0)
                b.loss.fill_(-7.0)
                b.inv.fill_(-7.0)
                assert old_call(handle, shape, b, ws, stream)() == 0
                torch.cuda.synchronize()
                got.append((b.loss.clone(), b.dl.clone(), b.inv.clone()))
            eq = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(*got))
            same_bits = same_bits and eq
            say(f"# default call {'x'.join(map(str, shape))}: loss {got[0][0].item():.9g}, loss / gradient / inverse count bit-identical "
                f"to the parent's build: {eq}")
        result["bit_identical"] = same_bits
        result["default_not_slower"] = worst <= 0.0

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
