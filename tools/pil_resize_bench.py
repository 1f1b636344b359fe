"""Pillow's 8-bit resize on the device (csrc/pil_resize.hip) against the host's Image.resize; prints text lines, then one
JSON line.  Every figure is taken after warm-up, from device events or from a host clock that ends in a synchronise.
  (a) kernel    ops.pil_resize alone on a Pet-like mix (--n images, sides drawn from 200..600, BICUBIC to 224 x 224 and
                BILINEAR to 256 x 256, 3 channels): us per image; bytes = source + output once each, computed from the
                shapes; bytes / time as a share of the HBM peak (--hbm-tbs, 8 TB/s for an MI355X).
  (b) host      Image.resize of the same mix with 1 and 16 threads: us per image (wall clock).
  (c) build     DevicePetDataset over a synthetic tree of --images JPEGs with sides from the same mix: resize="host" and
                resize="device" alternated (H D H D H D) in one process: ms per image, mean and spread (max - min) of
                each.  The device build counts as faster only if the means differ by more than the larger spread."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def mix_sizes(n, seed=0):
    """(h, w) pairs with all sides within 200..600: the long side drawn from 400..600, the short one from 200..550, one
    image in eight upright - a mean of about 385 x 485 (h x w), near the Pet's typical 375 x 500."""
    rng = np.random.default_rng(seed)
    sizes = []
    for i in range(n):
        long_side = int(rng.integers(400, 601))
        short_side = int(rng.integers(200, 551))
        short_side = min(short_side, long_side)
        sizes.append((short_side, long_side) if i % 8 else (long_side, short_side))
    return sizes


def texture(h, w, i, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 60 * np.sin(xx / (7.0 + i % 5) + c) * np.cos(yy / (11.0 + i % 3)) + rng.normal(0, 10, (h, w))
                    for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


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


def synthetic_tree(root, n, workers=16):
    base = os.path.join(root, "oxford-iiit-pet")
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "annotations", "trimaps"))
    sizes = mix_sizes(n, seed=1)

    def write(i):
        h, w = sizes[i]
        rng = np.random.default_rng(i)
        yy, xx = np.mgrid[0:h, 0:w]
        tri = np.where((yy - h // 2) ** 2 + (xx - w // 2) ** 2 < (min(h, w) // 3) ** 2, 1, 2).astype(np.uint8)
        Image.fromarray(texture(h, w, i, rng)).save(os.path.join(base, "images", f"pet_{i}.jpg"))
        Image.fromarray(tri).save(os.path.join(base, "annotations", "trimaps", f"pet_{i}.png"))

    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(write, range(n)))
    with open(os.path.join(base, "annotations", "trainval.txt"), "w") as f:
        f.writelines(f"pet_{i} {1 + i % 37} 1 1\n" for i in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    a = ap.parse_args()
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DevicePetDataset
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    dev = torch.device("cuda:0")
    res = {"n": a.n}
    sizes = mix_sizes(a.n)
    rng = np.random.default_rng(0)
    arrays = [texture(h, w, i, rng) for i, (h, w) in enumerate(sizes)]
    mean_h, mean_w = np.mean([s[0] for s in sizes]), np.mean([s[1] for s in sizes])
    print(f"mix: {a.n} images, mean {mean_h:.0f} x {mean_w:.0f}, sides {min(min(s) for s in sizes)}..{max(max(s) for s in sizes)}",
          flush=True)

    # (a) the kernel alone
    flat, shapes, offsets = ops.pil_pack(arrays, 3)
    src = torch.from_numpy(flat).to(dev)
    lut = torch.arange(256, dtype=torch.uint8).float().div(255).repeat(3, 1).contiguous().to(dev)
    for name, filt, size in (("bicubic_224", ops.PIL_BICUBIC, (224, 224)), ("bilinear_256", ops.PIL_BILINEAR, (256, 256))):
        desc = torch.from_numpy(ops.pil_describe(shapes, offsets, size, filt, dev).view(np.uint8)).to(dev)
        out = torch.empty(a.n, 3, *size, dtype=torch.uint8, device=dev)
        out_f = torch.empty(a.n, 3, *size, dtype=torch.float32, device=dev)
        for kind, kw, out_bytes in (("u8", dict(out=out), out.numel()), ("f32", dict(out_f32=out_f, lut=lut), out_f.numel() * 4)):
            ms = timed(lambda: ops.pil_resize(src, desc, 3, size, **kw), a.warmup, a.steps)
            nbytes = flat.size + out_bytes
            share = nbytes / (ms * 1e-3) / (a.hbm_tbs * 1e12)
            res[f"kernel_{name}_{kind}_us_per_image"] = round(ms * 1e3 / a.n, 3)
            res[f"kernel_{name}_{kind}_hbm_share"] = round(share, 4)
            print(f"(a) kernel {name} -> {kind}: {ms * 1e3 / a.n:.3f} us/image ({ms:.3f} ms per launch of {a.n}); "
                  f"{nbytes / 1e6:.1f} MB read + written = {nbytes / ms / 1e6:.1f} GB/s = {100 * share:.2f} % of the "
                  f"{a.hbm_tbs:g} TB/s HBM peak", flush=True)

    # (b) host Pillow on the same mix
    pil = [Image.fromarray(x) for x in arrays]
    for name, filt, size in (("bicubic_224", Image.BICUBIC, (224, 224)), ("bilinear_256", Image.BILINEAR, (256, 256))):
        for threads in (1, 16):
            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(lambda im: im.resize(size, filt), pil[:32]))
                t = time.perf_counter()
                list(ex.map(lambda im: im.resize(size, filt), pil))
                us = (time.perf_counter() - t) * 1e6 / a.n
            res[f"host_{name}_{threads}t_us_per_image"] = round(us, 1)
            print(f"(b) host Pillow {name}, {threads} thread(s): {us:.1f} us/image", flush=True)

    # (c) the dataset build, host and device alternated
    with tempfile.TemporaryDirectory() as tmp:
        t = time.perf_counter()
        synthetic_tree(tmp, a.images)
        print(f"synthetic tree of {a.images} JPEGs written in {time.perf_counter() - t:.1f} s", flush=True)
        src_ds = download_data(tmp, "trainval")
        DevicePetDataset(src_ds, device=dev, resize="device")                      # warm-up: file cache, tables, allocator
        torch.cuda.synchronize()
        runs = {"host": [], "device": []}
        check = {}
        for rep in range(3):
            for mode in ("host", "device"):
                t = time.perf_counter()
                ds = DevicePetDataset(src_ds, device=dev, resize=mode)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t) * 1e3 / a.images
                runs[mode].append(ms)
                check[mode] = (ds.images, ds.trimaps)
                print(f"(c) build {rep} resize={mode}: {ms:.3f} ms/image", flush=True)
        equal = all(torch.equal(x, y) for x, y in zip(check["host"], check["device"]))
    for mode, v in runs.items():
        res[f"build_{mode}_ms_per_image"] = [round(x, 4) for x in v]
        res[f"build_{mode}_mean"] = round(float(np.mean(v)), 4)
        res[f"build_{mode}_spread"] = round(max(v) - min(v), 4)
    gap = res["build_host_mean"] - res["build_device_mean"]
    bar = max(res["build_host_spread"], res["build_device_spread"])
    res["build_equal"] = equal
    res["build_images"] = a.images
    res["device_build_faster"] = bool(gap > bar)
    print(f"(c) host {res['build_host_mean']:.3f} ms/image (spread {res['build_host_spread']:.3f}), device "
          f"{res['build_device_mean']:.3f} ms/image (spread {res['build_device_spread']:.3f}); difference {gap:.3f} vs the larger "
          f"spread {bar:.3f}: device build {'FASTER' if gap > bar else 'NOT faster'}; tensors equal: {equal}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
