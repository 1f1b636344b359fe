"""Fully-supervised baseline throughput (FullySupervisedModel/SupervisedModel.py on the device); prints one JSON line:
  train_img_s        planned train_step of the aux-less DeepLabV3-ResNet50 (CrossEntropy + Adam) at B x 224 x 224
  eval_img_s         eval-mode forward + wsdl_seg_counts at B x 224 x 224
  count_us           wsdl_seg_counts alone at B x 2 x 224 x 224
  build_ms_per_img   DevicePetDataset construction (decode + resize on the host thread pool, copy to the device) per image
                     of a synthetic tree of --images JPEGs of 500 x 375 (the Pet's typical size)
Device times: CUDA events around --steps calls after --warmup."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps          # ms per call


def synthetic_tree(root, n):
    from PIL import Image
    base = os.path.join(root, "oxford-iiit-pet")
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "annotations", "trimaps"))
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:375, 0:500]
    lines = []
    for i in range(n):
        tri = np.where((yy - 180) ** 2 + (xx - 250 - i) ** 2 < 120 ** 2, 1, 2).astype(np.uint8)
        img = np.stack([128 + 60 * np.sin(xx / (7.0 + i % 5) + c) + rng.normal(0, 10, tri.shape) for c in range(3)], -1)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(base, "images", f"pet_{i}.jpg"))
        Image.fromarray(tri).save(os.path.join(base, "annotations", "trimaps", f"pet_{i}.png"))
        lines.append(f"pet_{i} {1 + i % 37} 1 1\n")
    with open(os.path.join(base, "annotations", "trainval.txt"), "w") as f:
        f.writelines(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--images", type=int, default=256)
    a = ap.parse_args()
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DevicePetDataset
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer, train_step
    dev = torch.device("cuda:0")
    B, S = a.batch, 224
    torch.manual_seed(0)
    model = initialize_model(2, device=dev).train()
    opt = make_optimizer(model, lr=1e-4)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.rand(B, 3, S, S, device=dev)
    y = (torch.rand(B, S, S, device=dev) > 0.5).long()
    train_ms = timed(lambda: train_step(model, opt, x, y, criterion=crit), a.warmup, a.steps)
    st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
    planned = st is not None and st.disabled is None and st.replays > 0
    model.eval()
    row = torch.zeros(3 * 2 + 1, dtype=torch.int64, device=dev)

    def eval_batch():
        with torch.no_grad():
            ops.seg_counts(model(x)["out"], y, out=row, accumulate=True)
    eval_ms = timed(eval_batch, a.warmup, a.steps)
    logits = torch.randn(B, 2, S, S, device=dev)
    count_ms = timed(lambda: ops.seg_counts(logits, y, out=row, accumulate=True), a.warmup, a.steps * 10)
    with tempfile.TemporaryDirectory() as tmp:
        synthetic_tree(tmp, a.images)
        src = download_data(tmp, "trainval")
        t = time.perf_counter()
        DevicePetDataset(src, device=dev)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t
    print(json.dumps({"batch": B, "size": S, "train_img_s": round(B / train_ms * 1e3, 1), "train_planned": planned,
                      "eval_img_s": round(B / eval_ms * 1e3, 1), "count_us": round(count_ms * 1e3, 2),
                      "build_ms_per_img": round(build_s * 1e3 / a.images, 3), "build_images": a.images}), flush=True)


if __name__ == "__main__":
    main()
