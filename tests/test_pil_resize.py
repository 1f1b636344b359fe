"""Pillow's 8-bit resampling on the device (csrc/pil_resize.hip, ops.pil_resize) and what is built on it: the raw Pet
reader, the device-side dataset build, the item loader, the stage-2 image transforms and the exact stage hand-off.

The tolerance everywhere is zero differing bytes / bit-identical floats, and the reference of every comparison is Pillow itself
(or image_to_tensor / load_u8 / PseudoSegmentationDataset, which are Pillow) - never the kernel's own output.  Sources are
the closed-form patterns of tests/pil_resize_oracle.py."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_oracle as O  # noqa: E402
from conftest import report_line  # noqa: E402

FILTER_NAME = {O.BICUBIC: "bicubic", O.BILINEAR: "bilinear"}


def pillow(img, size, filt):
    return np.asarray(Image.fromarray(img).resize((size[1], size[0]), filt))


def normalize_lut():
    """ToTensor + Normalize per 8-bit value, computed the way image_to_tensor computes it (torch on the CPU)."""
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import _MEAN, _STD
    v = torch.arange(256, dtype=torch.uint8).float().div(255.0)
    return ((v.view(1, 256) - _MEAN.view(3, 1)) / _STD.view(3, 1)).contiguous()


def to_tensor_lut(c):
    return torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).repeat(c, 1).contiguous()


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_oracle_equals_live_pillow_and_the_fixture(golden):
    g = golden("pil_resize")
    made_with = str(g["pillow_version"])
    import PIL
    worst = 0
    for h, w in O.SIZES:
        for c in (1, 3):
            img = O.pattern(h, w, c)
            for filt, size in O.TARGETS:
                name = f"{h}x{w}x{c}_{FILTER_NAME[filt]}"
                got = O.resize(img, size, filt)
                live = pillow(img, size, filt)
                diff = int((got != live).sum())
                worst = max(worst, diff)
                assert diff == 0, f"{name}: oracle differs from Pillow {PIL.__version__} in {diff} bytes"
                digest = hashlib.sha256(got.tobytes()).hexdigest()
                assert digest == str(g["sha256/" + name]), (
                    f"{name}: Pillow {PIL.__version__} here resamples differently from Pillow {made_with}, which made the fixture")
                if "full/" + name in g.files:
                    assert np.array_equal(got, g["full/" + name]), name
    # the saturated block drives BICUBIC past both ends of the clamp: the un-clamped sum leaves [0, 255]
    img = O.pattern(375, 500, 1)
    _, bounds, kk = O.coeffs(500, 224, O.BICUBIC)
    acc = [(1 << 21) + int((img[r, b[0]:b[0] + b[1]].astype(np.int64) * k[:b[1]]).sum()) >> 22
           for r in (100, 200) for b, k in zip(bounds, kk)]
    assert min(acc) < 0 and max(acc) > 255
    report_line(f"pil_resize oracle vs Pillow {PIL.__version__}: {worst} differing bytes over {len(O.SIZES) * 4} cases")


def test_library_coefficients_equal_the_oracles():
    """wsdl_pil_coeffs (host only) against the numpy restatement: ksize, every bound, every coefficient."""
    from weaklysuperviseddl_amd import ops, WsdlError
    n = 0
    for n_in in list(range(1, 1101)) + [2500, 3000, 4096]:
        for n_out in (224, 256):
            for filt in (O.BILINEAR, O.BICUBIC):
                ksize, bounds, kk = ops.pil_coeffs(n_in, n_out, filt)
                want = O.coeffs(n_in, n_out, filt)
                assert ksize == want[0], (n_in, n_out, filt)
                assert np.array_equal(bounds, want[1]), (n_in, n_out, filt)
                assert np.array_equal(kk, want[2]), (n_in, n_out, filt)
                assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ksize).all()
                n += 1
    assert n == 1103 * 4
    # a pass whose in == out is the identity: 2^22 on the pixel itself, zeros beside it
    for filt in (O.BILINEAR, O.BICUBIC):
        _, bounds, kk = ops.pil_coeffs(224, 224, filt)
        for i in range(224):
            row = np.zeros(kk.shape[1], dtype=np.int32)
            row[i - bounds[i, 0]] = 1 << 22
            assert np.array_equal(kk[i], row)
    for bad in ((0, 224, O.BICUBIC), (224, 0, O.BICUBIC), (16385, 224, O.BILINEAR), (224, 16385, O.BILINEAR), (224, 224, 0),
                (224, 224, 1), (224, 224, 4), (-3, 224, O.BICUBIC)):
        with pytest.raises(WsdlError, match="pil_coeffs"):
            ops.pil_coeffs(*bad)
    assert ops.pil_coeffs(16384, 1, O.BICUBIC)[0] == 65537 and ops.pil_coeffs(1, 16384, O.BILINEAR)[0] == 3
    # and the device entry point refuses host tensors: no CPU fallback
    with pytest.raises(WsdlError):
        ops.pil_resize(torch.zeros(12, dtype=torch.uint8), np.zeros(1, dtype=ops.PIL_IMAGE_DTYPE), 3, (224, 224))


def make_pet_tree(root, n_trainval, n_test, lo=90, hi=1400):
    """A synthetic Oxford-IIIT Pet tree from closed-form patterns: sides lo..hi (up-sampling, width 224, height 224, large
    images), a grayscale JPEG and a palette-mode trimap among them."""
    base = root / "oxford-iiit-pet"
    (base / "images").mkdir(parents=True)
    (base / "annotations" / "trimaps").mkdir(parents=True)
    k = 0
    for split, n in (("trainval", n_trainval), ("test", n_test)):
        lines = []
        for i in range(n):
            name = f"{'Abyssinian' if i % 2 else 'boxer'}_{split}_{i}"
            h = lo + (k * 577) % (hi - lo + 1)
            w = lo + (k * 811 + 300) % (hi - lo + 1)
            if k % 9 == 1:
                w = 224
            if k % 9 == 2:
                h = 224
            if k % 13 == 3:
                h, w = hi, hi - 77
            img = O.pattern(h, w, 3)
            yy, xx = np.mgrid[0:h, 0:w]
            tri = (1 + ((xx * 5 // w) + (yy * 3 // h)) % 3).astype(np.uint8)
            image = Image.fromarray(img[:, :, 0]) if k % 7 == 4 else Image.fromarray(img)      # "L" JPEG now and then
            image.save(base / "images" / f"{name}.jpg", quality=85)
            t = Image.fromarray(tri)
            if k % 11 == 5:
                t = t.convert("P")                                                              # palette-mode trimap
            t.save(base / "annotations" / "trimaps" / f"{name}.png")
            lines.append(f"{name} {1 + (k * 7) % 37} {1 + i % 2} {1 + i % 12}\n")
            k += 1
        (base / "annotations" / f"{split}.txt").write_text("".join(lines))
    return root


def test_load_raw_resized_by_pillow_is_load_u8(tmp_path):
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    root = make_pet_tree(tmp_path / "pet", 12, 2, lo=90, hi=400)
    ds = download_data(pth=str(root), split="trainval")
    modes = set()
    for i in range(len(ds)):
        img, cat, tri = ds.load_raw(i)
        want_img, want_cat, want_tri = ds.load_u8(i)
        modes.add((Image.open(ds._images[i]).mode, Image.open(ds._segs[i]).mode))
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and tri.dtype == np.uint8 and tri.ndim == 2
        assert img.shape[:2] == Image.open(ds._images[i]).size[::-1] and cat == want_cat
        if Image.open(ds._segs[i]).mode != "L":
            assert tri.shape == (224, 224)                      # resized on the host (Pillow forces NEAREST for "P")
        else:
            assert tri.shape == img.shape[:2]
        assert np.array_equal(pillow(img, (224, 224), O.BICUBIC), want_img)
        assert np.array_equal(pillow(tri, (224, 224), O.BICUBIC), want_tri)
    assert ("L", "L") in modes and ("RGB", "P") in modes and ("RGB", "L") in modes


def test_item_loader_batches_on_cpu_tensors():
    """DeviceItemLoader's batching on a stand-in dataset of CPU tensors: what DataLoader collates, partial batch included."""
    from types import SimpleNamespace
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DeviceItemLoader, _to_float_table
    n = 13
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, 3, 224, 224), dtype=torch.uint8, generator=g)
    trimaps = torch.randint(1, 4, (n, 224, 224), dtype=torch.uint8, generator=g)
    cats = torch.arange(n, dtype=torch.int64) * 3 % 37

    class Stub(SimpleNamespace):
        def __len__(self):
            return n

    ds = Stub(images=images, trimaps=trimaps, categories=cats, _table=_to_float_table(), device=torch.device("cpu"))
    loader = DeviceItemLoader(ds, 5)
    batches = list(loader)
    assert len(loader) == 3 and [b[0].shape[0] for b in batches] == [5, 5, 3]
    for k, (x, (c, t)) in enumerate(batches):
        sl = slice(5 * k, 5 * k + 5)
        assert x.dtype == torch.float32 and torch.equal(x, images[sl].to(torch.float32).div(255))
        assert c.dtype == torch.int64 and torch.equal(c, cats[sl])
        assert t.dtype == torch.uint8 and t.shape[1:] == (1, 224, 224) and torch.equal(t[:, 0], trimaps[sl])
    sub = list(DeviceItemLoader(ds, 4, indices=[7, 2, 9]))
    assert len(sub) == 1 and torch.equal(sub[0][1][0], cats[[7, 2, 9]])
    a = [b[1][0] for b in DeviceItemLoader(ds, 5, shuffle=True, generator=torch.Generator().manual_seed(3))]
    assert torch.equal(torch.cat(a), cats[torch.randperm(n, generator=torch.Generator().manual_seed(3))])


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("filt,size", O.TARGETS)
def test_kernel_equals_pillow_on_mixed_sizes_in_one_launch(dev, filt, size, c):
    from weaklysuperviseddl_amd import ops
    images = [O.pattern(h, w, c) for h, w in O.SIZES]
    want = np.stack([pillow(im, size, filt).reshape(size[0], size[1], c).transpose(2, 0, 1) for im in images])
    lut = to_tensor_lut(c) if filt == O.BICUBIC or c == 1 else normalize_lut()
    out = torch.empty(len(images), c, *size, dtype=torch.uint8, device=dev)
    out_f = torch.empty(len(images), c, *size, dtype=torch.float32, device=dev)
    got, got_f = ops.pil_resize_arrays(images, size, filt, channels=c, device=dev, out=out, out_f32=out_f, lut=lut.to(dev))
    assert got is out and got_f is out_f
    diff = int((got.cpu().numpy() != want).sum())
    report_line(f"pil_resize {FILTER_NAME[filt]} C={c}: {diff} of {want.size} bytes differ from Pillow ({len(images)} sizes, one launch)")
    assert diff == 0
    # the float epilogue against the host transforms
    if c == 3 and filt == O.BILINEAR:
        from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import image_to_tensor
        ref_f = torch.stack([image_to_tensor(Image.fromarray(im), size) for im in images])
    else:                                                                  # ToTensor
        ref_f = torch.from_numpy(want).to(torch.float32).div(255)
    assert torch.equal(got_f.cpu(), ref_f)
    # uint8 alone, float alone, a second run: the same bits
    again, none = ops.pil_resize_arrays(images, size, filt, channels=c, device=dev)
    assert none is None and torch.equal(again, got)
    _, f_only = ops.pil_resize_arrays(images, size, filt, channels=c, device=dev, out_f32=torch.empty_like(out_f), lut=lut.to(dev))
    assert torch.equal(f_only, got_f)
    # one image alone equals its bytes inside the mixed batch
    for i in (0, 5, 7, len(images) - 1):
        alone, _ = ops.pil_resize_arrays([images[i]], size, filt, channels=c, device=dev)
        assert torch.equal(alone[0], got[i]), O.SIZES[i]


@pytest.mark.gpu
def test_pil_resize_refuses_bad_arguments(dev):
    from weaklysuperviseddl_amd import ops, WsdlError
    img = O.pattern(20, 30, 3)
    with pytest.raises(WsdlError):
        ops.pil_resize_arrays([img], (224, 224), 0, device=dev)                       # NEAREST is not part of this
    with pytest.raises(WsdlError):
        ops.pil_resize_arrays([img], (224, 224), O.BICUBIC, channels=2, device=dev)
    with pytest.raises(WsdlError):
        ops.pil_resize_arrays([img], (0, 224), O.BICUBIC, device=dev)
    with pytest.raises(WsdlError):
        ops.pil_resize_arrays([img], (224, 16385), O.BICUBIC, device=dev)
    with pytest.raises(WsdlError):
        ops.pil_resize_arrays([img.astype(np.float32)], (224, 224), O.BICUBIC, device=dev)
    src = torch.from_numpy(img.reshape(-1)).to(dev)
    desc = ops.pil_describe([(20, 30)], [0], (224, 224), O.BICUBIC, dev)
    with pytest.raises(WsdlError, match="outside"):
        ops.pil_resize(src[:-1].contiguous(), desc, 3, (224, 224))
    with pytest.raises(WsdlError, match="lut"):
        ops.pil_resize(src, desc, 3, (224, 224), out_f32=torch.empty(1, 3, 224, 224, device=dev))
    with pytest.raises(WsdlError):
        ops.pil_resize(src, desc, 3, (224, 224), out=torch.empty(1, 3, 224, 200, dtype=torch.uint8, device=dev))


@pytest.fixture(scope="module")
def pet_tree(tmp_path_factory):
    return make_pet_tree(tmp_path_factory.mktemp("pet"), 41, 13)


@pytest.mark.gpu
def test_device_build_equals_host_build(dev, pet_tree):
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DevicePetDataset
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    src = download_data(pth=str(pet_tree), split="trainval")
    assert len(src) >= 40
    sides = [Image.open(p).size for p in src._images]
    assert min(min(s) for s in sides) < 224 < 1400 <= max(max(s) for s in sides) and any(s[0] == 224 for s in sides)
    host = DevicePetDataset(src, device=dev, workers=4)
    # 3 MB per chunk: several chunks, and single items larger than the bound (1400 x 1323 x 4 bytes) among them
    small = DevicePetDataset(src, device=dev, workers=4, resize="device", chunk_bytes=3 << 20)
    default = DevicePetDataset(src, device=dev, workers=4, resize="device")
    for name, got in (("3 MB chunks", small), ("default chunks", default)):
        for field in ("images", "trimaps", "categories"):
            a, b = getattr(got, field), getattr(host, field)
            assert a.dtype == b.dtype and a.shape == b.shape
            diff = int((a != b).sum())
            report_line(f"DevicePetDataset(resize='device', {name}).{field}: {diff} of {b.numel()} values differ from resize='host'")
            assert diff == 0, (name, field)
    with pytest.raises(ValueError):
        DevicePetDataset(src, device=dev, resize="gpu")


@pytest.mark.gpu
def test_item_loader_equals_the_host_dataloader_and_feeds_stage_one(dev, pet_tree):
    from torch.utils.data import DataLoader
    from weaklysuperviseddl_amd.FullySupervisedModel.PetDataset import DevicePetDataset, DeviceItemLoader
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks
    from weaklysuperviseddl_amd.TraditionalModel.ExtraUtilities import download_data
    from test_hip_dp import _cam_generator
    src = download_data(pth=str(pet_tree))                                   # 13 test items: 5 + 5 + 3
    host_loader = DataLoader(src, batch_size=5)
    dev_loader = DeviceItemLoader(DevicePetDataset(src, device=dev, workers=4, resize="device"), 5)
    want, got = list(host_loader), list(dev_loader)
    assert len(want) == len(got) == len(dev_loader) == 3
    for (x, (c, t)), (dx, (dc, dt)) in zip(want, got):
        assert dx.is_cuda and dx.dtype == x.dtype and torch.equal(dx.cpu(), x)
        assert dc.dtype == c.dtype == torch.int64 and torch.equal(dc.cpu(), c)
        assert dt.dtype == t.dtype == torch.uint8 and dt.shape == t.shape and torch.equal(dt.cpu(), t)
    gen = _cam_generator(dev)
    generate_pseudo_masks(host_loader, gen, cam_thresh=0.3, write_png=False, device=dev)
    ids, masks = generate_pseudo_masks.last_ids, [np.array(m) for m in generate_pseudo_masks.last_masks]
    generate_pseudo_masks(dev_loader, gen, cam_thresh=0.3, write_png=False, device=dev)
    assert generate_pseudo_masks.last_ids == ids and len(masks) == 13
    for a, b in zip(masks, generate_pseudo_masks.last_masks):
        assert np.array_equal(a, np.asarray(b))
    assert sum(int(m.sum()) for m in masks) > 0


@pytest.mark.gpu
def test_stage_two_transforms_on_the_device(dev, tmp_path):
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationDataset import (InMemoryPseudoDataset, PseudoSegmentationDataset,
                                                                            image_to_tensor, images_to_tensor_device)
    img_dir, mask_dir = tmp_path / "images", tmp_path / "pseudo_masks"
    img_dir.mkdir()
    mask_dir.mkdir()
    sizes = [(224, 224), (375, 500), (137, 91), (256, 256), (300, 224), (600, 411), (1, 37)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(O.pattern(h, w, 3)).save(img_dir / f"{i}.png")
        yy, xx = np.mgrid[0:h, 0:w]
        Image.fromarray((((xx * 4 // w + yy * 3 // max(h, 1)) % 2) * 255).astype(np.uint8)).save(mask_dir / f"{i}.png")
    pil_images = [Image.fromarray(O.pattern(h, w, 3)) for h, w in sizes]
    want = torch.stack([image_to_tensor(im) for im in pil_images])
    assert torch.equal(images_to_tensor_device(pil_images, device=dev).cpu(), want)
    assert torch.equal(images_to_tensor_device([np.asarray(im) for im in pil_images], device=dev).cpu(), want)
    small = torch.stack([image_to_tensor(im, (96, 128)) for im in pil_images])
    assert torch.equal(images_to_tensor_device(pil_images, (96, 128), device=dev).cpu(), small)
    ref = PseudoSegmentationDataset(str(img_dir), str(mask_dir), transform=True, return_name=True)
    mem = InMemoryPseudoDataset.from_dirs(str(img_dir), str(mask_dir), device=dev, chunk=3)
    assert len(mem) == len(ref) == len(sizes)
    for k in range(len(ref)):
        (a, m, name), (b, n, nm) = ref[k], mem[k]
        assert name == nm and torch.equal(b.cpu(), a) and n.dtype == m.dtype and torch.equal(n.cpu(), m)


@pytest.mark.gpu
def test_exact_stage_handoff_equals_the_png_round_trip(dev, tmp_path):
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks, stage_handoff, PseudoSegmentationDataset
    from test_hip_dp import _cam_generator, _cam_loader
    gen = _cam_generator(dev)
    img_dir, mask_dir = generate_pseudo_masks(_cam_loader(2, 3), gen, cam_thresh=0.3, out_root=str(tmp_path), run_id="t",
                                              write_png=True, keep_images=True)
    masks, images = generate_pseudo_masks.last_masks, torch.stack(generate_pseudo_masks.last_images)
    im256, m256 = stage_handoff(images, masks, (256, 256), dev, exact=True)
    ds = PseudoSegmentationDataset(img_dir, mask_dir, transform=True, return_name=True)
    order = sorted(range(6), key=lambda i: f"{i}.png")
    differing = 0
    for k, i in enumerate(order):
        img, mask, name = ds[k]
        assert name == f"{i}.png"
        differing += int((im256[i].cpu() != img).sum())
        assert torch.equal(m256[i].cpu().long(), mask)
    report_line(f"stage_handoff(exact=True): {differing} of {im256.numel()} floats differ from the PNG round trip")
    assert differing == 0
    # the default is unchanged: the float up-sampler, within one 8-bit level
    im_default, m_default = stage_handoff(images, masks, (256, 256), dev)
    assert torch.equal(m_default, m256) and (im_default - im256).abs().max().item() <= 1.0 / 255 / 0.224 + 1e-5
