"""Dense-CRF refinement throughput: device ms/img of ops.dense_crf at 224 x 224 for B = 1, 8, 32 (pydensecrf's
parameters, 5 iterations, cam in, masks out) and the CPU oracle's time per image (tests/crf_oracle.py, one image).
Device times: CUDA events around `--reps` calls after `--warmup`; median of the per-call times."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    from weaklysuperviseddl_amd import ops
    from conftest import smooth_image
    import crf_oracle as co
    S = a.size
    dev = torch.device("cuda:0")
    res = {}
    for B in [int(x) for x in a.batches.split(",")]:
        img = smooth_image(B, S, S, 0).to(dev)
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
        cam = torch.exp(-(xx ** 2 + yy ** 2) * 3).expand(B, S, S).contiguous().to(dev)
        for _ in range(a.warmup):
            ops.dense_crf(img, cam, cam_thresh=0.2)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.dense_crf(img, cam, cam_thresh=0.2)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        res[B] = ms / B
        print(f"device  B={B:3d}  {S}x{S}: {ms:8.3f} ms/call  {ms / B:7.3f} ms/img  (min {min(times) / B:.3f})", flush=True)
    if not a.no_oracle:
        x = smooth_image(1, S, S, 0)[0].numpy()
        rgb = co.quantise(x)
        cam = np.exp(-np.add.outer(np.linspace(-1, 1, S) ** 2, np.linspace(-1, 1, S) ** 2) * 3).astype(np.float32)
        t = time.perf_counter()
        co.dense_crf(rgb, cam, 0.2)
        dt = (time.perf_counter() - t) * 1e3
        print(f"oracle  B=  1  {S}x{S}: {dt:8.1f} ms/img (numpy, float64 filtering)", flush=True)


if __name__ == "__main__":
    main()
