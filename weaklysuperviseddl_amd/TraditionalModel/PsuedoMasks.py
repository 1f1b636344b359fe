"""Pseudo-mask generation on the HIP path.

Mirrors reference TraditionalModel/PsuedoMasks.py: ``keep_largest`` (:15-21) and
``generate_pseudo_masks`` (:23-79).  Differences, all outside the arithmetic:
  * CAM + threshold run batched on the device (``LayerCAMGenerator.generate_batch`` with the
    threshold fused into the epilogue kernel) - one device->host copy of uint8 masks per batch instead
    of a float map per image;
  * output directories are parameters (the reference hard-codes /content/...); ``write_png=False``
    keeps the masks in memory for the in-memory hand-off to stage 2
    (``generate_pseudo_masks.last_masks`` / ``.last_ids`` / ``.last_images``; ``stage_handoff`` turns them into
    what ``PseudoSegmentationDataset`` would have read back from the PNGs);
  * ``rank`` / ``world``: stage 1 is per-image independent (eval-mode BN), so under data parallelism the loader's
    batches are dealt round-robin to the ranks - batch j belongs to rank j % world - with NO collective
    (SURVEY.md 8e); image ids stay the global ones, so the union over the ranks is the single-process result;
  * ``streams``: that many of the loader's batches are in flight on the device at once (``LayerCAMGenerator.generate_batches``);
    the masks are the same bit for bit;
  * ``pamr``: optional pixel-adaptive refinement of the CAM before its threshold (``ops.pamr``; off by default);
  * ``superpixels``: optional snapping of the CAM, before its threshold, to the means over SLIC superpixels of the batch's
    images (``ops.slic`` + ``ops.superpixel_snap``; off by default);
  * ``affinity``: optional random walk of the CAM, before its threshold, under the learned affinities of an ``AffinityNet``
    (``ops.affinity_random_walk``; off by default);
  * ``boundary``: optional random walk of the CAM, before its threshold, under the boundary-path affinities of a
    ``BoundaryNet`` (``ops.edge_random_walk``; off by default);
  * ``generate_prototype_pseudo_masks``: optional prototype CAM - the softmax similarity of every pixel's features to the image's own foreground and
    background prototypes, pooled over the CAM's sure regions (``prototype_cam``; off by default);
  * ``generate_adaptive_pseudo_masks``: optional threshold per image - Otsu's, from a histogram of the map on the device - in place
    of ``cam_thresh`` (``adaptive_masks``; off by default);
  * ``keep_largest(mask)`` is the reference's host function (skimage there; scipy.ndimage here - 8-connectivity, raster
    label order, first label wins area ties, empty mask returned unchanged).  ``generate_pseudo_masks`` itself labels
    the whole batch on the device (``keep_largest_batched`` -> ``ops.keep_largest_batched``, one workgroup per mask, the
    same result bit for bit): one device->host copy of the FINAL masks per batch, and none at all with
    ``keep_on_device=True`` - the in-memory hand-off to stage 2 then never synchronises with the host.
"""
import os

import numpy as np
import torch
from scipy import ndimage

from .. import ops

_EIGHT = np.ones((3, 3), dtype=bool)


def keep_largest(mask):
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=_EIGHT)
    if n == 0:
        return mask
    areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return (lab == (int(np.argmax(areas)) + 1)).astype(np.uint8)


def _to_device_async(t, device):
    """Host tensors go through pinned memory: a copy from pageable memory makes the host wait until the stream has
    drained - one such copy per batch (the labels) serialised stage 1 with whatever the device was still running."""
    if t.is_cuda or torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def keep_largest_batched(masks):
    """``keep_largest`` for a (N,H,W) batch of uint8 device masks, on the device."""
    return ops.keep_largest_batched(masks)


def seeds_from_cam(cam, lo, hi, ignore_index=255):
    """Seeds for ``nn.SeededRegionGrowingLoss`` from a CAM in [0, 1] (the reference has no such step): int64, 1 where
    ``cam >= hi`` (sure foreground), 0 where ``cam <= lo`` (sure background), ``ignore_index`` between - and at a NaN.
    Plain tensor operations on the CAM's device.  Seeds that go through ``train_step`` need a negative ``ignore_index``
    (it clamps its masks to at most 1, as the reference does)."""
    if not lo < hi:
        raise ValueError(f"seeds_from_cam: lo {lo!r} must be below hi {hi!r}")
    cam = torch.as_tensor(cam)
    seeds = torch.full(cam.shape, int(ignore_index), dtype=torch.int64, device=cam.device)
    seeds = torch.where(cam <= lo, torch.zeros_like(seeds), seeds)
    return torch.where(cam >= hi, torch.ones_like(seeds), seeds)


def superpixel_cam(images, cam, **slic_kwargs):
    """A CAM (B,H,W) snapped to the SLIC superpixels of ``images`` (B,3,H,W), float (ImageNet-normalised: ``ops.slic_quantize``)
    or uint8: every pixel gets the mean of the CAM over its superpixel.  ``slic_kwargs`` are the keywords of ``ops.slic``."""
    step, _, _, min_size = ops.check_slic_options(**dict(slic_kwargs, name="superpixel_cam"))
    if images.is_floating_point():
        images = ops.slic_quantize(images)
    segments, _ = ops.slic(images, **slic_kwargs)
    n_max = ops.slic_max_segments(cam.shape[-2], cam.shape[-1], step, min_size)
    return ops.superpixel_snap(cam[:, None].float(), segments, n_max)[:, 0]


def _affinity_options(affinity):
    """The ``affinity=`` dict of ``generate_pseudo_masks`` with its defaults; ValueError / WsdlError for what it cannot be."""
    if not isinstance(affinity, dict) or "net" not in affinity or set(affinity) - {"net", "radius", "beta", "num_iter"}:
        raise ValueError("generate_pseudo_masks: affinity= is a dict of net, radius, beta, num_iter (net is required)")
    opts = dict(radius=5, beta=8.0, num_iter=256)
    opts.update(affinity)
    ops.check_affinity_options(opts["radius"], beta=opts["beta"], num_iter=opts["num_iter"], name="generate_pseudo_masks: affinity")
    return opts


def affinity_cam(images, cam, net, radius=5, beta=8.0, num_iter=256):
    """A CAM (B,H,W) propagated by AffinityNet's random walk: resized to the feature size of ``net(images)``, walked ``num_iter``
    steps as a one-channel map under ``ops.affinity_transitions(ops.pair_affinity(features), beta)``, resized back to H x W."""
    with torch.no_grad():
        feat = net(images)
    small = ops.bilinear_resize(cam[:, None].float().contiguous(), tuple(feat.shape[-2:]))
    walked = ops.affinity_random_walk(feat, small, radius=radius, beta=beta, num_iter=num_iter)
    return ops.bilinear_resize(walked, tuple(cam.shape[-2:]))[:, 0]


def _boundary_options(boundary):
    """The ``boundary=`` dict of ``generate_pseudo_masks`` with its defaults; ValueError / WsdlError for what it cannot be."""
    if not isinstance(boundary, dict) or "net" not in boundary or set(boundary) - {"net", "radius", "beta", "num_iter"}:
        raise ValueError("generate_pseudo_masks: boundary= is a dict of net, radius, beta, num_iter (net is required)")
    opts = dict(radius=5, beta=10.0, num_iter=256)
    opts.update(boundary)
    ops.check_path_affinity_options(opts["radius"], beta=opts["beta"], num_iter=opts["num_iter"], name="generate_pseudo_masks: boundary")
    return opts


def boundary_cam(images, cam, net, radius=5, beta=10.0, num_iter=256):
    """A CAM (B,H,W) propagated by IRN's boundary walk: ``edge = sigmoid(net(images))`` (a ``BoundaryNet``, no gradient), the CAM
    resized to the edge size, ``ops.edge_random_walk`` as a one-channel map, resized back to H x W and divided by its per-image
    maximum + 1e-5 (IRN's renormalisation; tensor operations on the device)."""
    with torch.no_grad():
        edge = torch.sigmoid(net(images))
    small = ops.bilinear_resize(cam[:, None].float().contiguous(), tuple(edge.shape[-2:]))
    walked = ops.edge_random_walk(edge, small, radius=radius, beta=beta, num_iter=num_iter)
    back = ops.bilinear_resize(walked, tuple(cam.shape[-2:]))[:, 0]
    return back / (back.amax(dim=(-2, -1), keepdim=True) + 1e-5)


def _prototype_options(prototype):
    """The ``prototype`` dict of ``generate_prototype_pseudo_masks`` with its defaults; ValueError / WsdlError for what it cannot be."""
    if not isinstance(prototype, dict) or "net" not in prototype or set(prototype) - {"net", "lo", "hi", "temperature"}:
        raise ValueError("generate_prototype_pseudo_masks: prototype is a dict of net, lo, hi, temperature (net is required)")
    opts = dict(lo=0.05, hi=0.3, temperature=0.1)
    opts.update(prototype)
    if not opts["lo"] < opts["hi"]:
        raise ValueError(f"generate_prototype_pseudo_masks: lo {opts['lo']!r} must be below hi {opts['hi']!r}")
    ops.check_prototype_options(temperature=opts["temperature"], name="generate_prototype_pseudo_masks")
    return opts


def prototype_cam(images, cam, net, *, lo=0.05, hi=0.3, temperature=0.1):
    """A CAM (B,H,W) in [0, 1] replaced by its image-specific prototype CAM (SIPE, Chen et al., CVPR 2022): the features are
    ``net(images)`` (B,D,h,w), without a gradient; the seeds ``seeds_from_cam(cam, lo, hi)`` - 1 sure foreground, 0 sure background -
    are down-sampled to h x w by nearest neighbour; ``ops.class_prototypes`` pools one background and one foreground prototype per
    image; the result is the foreground channel of ``ops.prototype_similarity(..., activation='softmax', temperature=)``, resized
    back to H x W (``ops.bilinear_resize``).  An image without a background seed or without a foreground seed keeps its input CAM
    (a ``torch.where`` on the masses: no host read)."""
    with torch.no_grad():
        feat = net(images)
    seeds = seeds_from_cam(cam, lo, hi)
    iy = nearest_resize_index(feat.shape[-2], seeds.shape[1], seeds.device)
    ix = nearest_resize_index(feat.shape[-1], seeds.shape[2], seeds.device)
    proto, mass = ops.class_prototypes(feat, seeds[:, iy][:, :, ix].contiguous(), 2)
    sim = ops.prototype_similarity(feat, proto, activation="softmax", temperature=temperature)
    back = ops.bilinear_resize(sim[:, 1:2].contiguous(), tuple(cam.shape[-2:]))[:, 0]
    return torch.where((mass > 0).all(dim=1)[:, None, None], back, cam.float())


def _to_png_u8(t):
    """torchvision.utils.save_image's quantisation: mul(255).add_(0.5).clamp_(0, 255) -> uint8, HWC."""
    return t.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()


def generate_pseudo_masks(loader, layercam_gen, cam_thresh=0.3, alpha=1.0, keep_largest_masks=True,
                          run_id="default", out_root="/content", max_images=500, write_png=True,
                          device="cuda", rank=0, world=1, keep_images=False, streams=3, keep_on_device=False,
                          device_batch=0, pamr=None, superpixels=None, affinity=None, boundary=None, multiscale=None):
    """``multiscale``: None (the default: bit for bit the path without the argument) or a dict of keyword arguments of
    ``LayerCAMGenerator.generate_multiscale`` (``scales``, ``flip``, ``reduce``, ``multiple``; ``{}``: its defaults) - the CAM of every
    loader batch is the fusion over scales and the mirror image, divided by its per-image maximum; it takes the place of the CAM
    before ``pamr`` / ``superpixels`` / ``affinity`` / ``boundary`` and the threshold (``v >= cam_thresh and v > 0``).  One eager pass
    per loader batch and scale (``streams`` is not used, no hipGraph); ``device_batch > 0`` together with it is refused.  With the
    default split arithmetic an image's CAM depends on which images share its device batch (the per-tensor scale effect the README
    notes for coalesced CAMs): the masks depend on the loader's batches, and the mirrored half shares a batch with the plain half.

    ``pamr``: None (the default: the masks are the thresholded CAMs, bit for bit as without the argument) or a dict of
    keyword arguments of ``ops.pamr`` (``{}``: its defaults) - the CAM WITHOUT its threshold is refined against the batch's
    images as a one-channel score map (pixel-adaptive mask refinement; the reference has no such step), the refined map is
    thresholded (``>= cam_thresh``) and ``keep_largest`` applies as before.  The images must have the CAM's size.

    ``superpixels``: None (the default: bit for bit the path without the argument) or a dict of keyword arguments of ``ops.slic``
    (``step`` is required) - the CAM WITHOUT its threshold is replaced by its means over the SLIC superpixels of the batch's
    images (``superpixel_cam``; the reference has no such step), then ``>= cam_thresh``, then ``keep_largest`` as before.
    Combining it with ``pamr`` is refused.

    ``affinity``: None (the default: bit for bit the path without the argument) or a dict with ``net`` (an ``AffinityNet``, on the
    device, in eval mode) and optionally ``radius`` (5), ``beta`` (8.0) and ``num_iter`` (256) - the CAM WITHOUT its threshold is
    resized to the net's feature size (``ops.bilinear_resize``), walked as a one-channel map under the affinities of the batch's
    features (``affinity_cam``; the reference has no such step) and resized back, then ``>= cam_thresh``, then ``keep_largest``
    as before.  Combining it with ``pamr`` or ``superpixels`` is refused.

    ``boundary``: None (the default: bit for bit the path without the argument) or a dict with ``net`` (a ``BoundaryNet``, on the
    device, in eval mode) and optionally ``radius`` (5), ``beta`` (10.0) and ``num_iter`` (256) - the CAM WITHOUT its threshold is
    resized to the size of the net's boundary map, damped by ``1 - edge`` and walked as a one-channel map under the boundary-path
    affinities (``boundary_cam``; the reference has no such step), resized back and divided by its per-image maximum, then
    ``>= cam_thresh``, then ``keep_largest`` as before.  Combining it with ``pamr``, ``superpixels`` or ``affinity`` is refused."""
    return _generate_pseudo_masks(loader, layercam_gen, cam_thresh, alpha, keep_largest_masks, run_id, out_root, max_images, write_png,
                                  device, rank, world, keep_images, streams, keep_on_device, device_batch, pamr, superpixels, affinity,
                                  boundary, multiscale, None)


def generate_prototype_pseudo_masks(loader, layercam_gen, prototype, **kwargs):
    """``generate_pseudo_masks(loader, layercam_gen, **kwargs)`` with the prototype CAM in front of the threshold.  (A function of
    its own: the positional signature of ``generate_pseudo_masks`` is pinned.)  ``prototype``: None (bit for bit
    ``generate_pseudo_masks``) or a dict with ``net`` (a ``TrunkFeatures`` or a ``ProjectionNet``, on the device, in eval mode) and
    optionally ``lo`` (0.05), ``hi`` (0.3) and ``temperature`` (0.1) - the CAM WITHOUT its threshold is replaced by the prototype CAM
    of the batch's features (``prototype_cam``; the reference has no such step), then ``>= cam_thresh``, then ``keep_largest`` as
    before.  Combining it with ``pamr``, ``superpixels``, ``affinity`` or ``boundary`` is refused; ``multiscale`` may come first.  The
    results are left where ``generate_pseudo_masks`` leaves them (``generate_pseudo_masks.last_masks`` / ``.last_ids`` /
    ``.last_images``)."""
    return _generate_pseudo_masks(loader, layercam_gen, prototype=prototype, **kwargs)


def _adaptive_options(adaptive):
    """The ``adaptive`` dict of ``generate_adaptive_pseudo_masks`` with its defaults; ValueError / WsdlError for what it cannot be."""
    if not isinstance(adaptive, dict) or set(adaptive) - {"method", "bins", "floor", "ceil"}:
        raise ValueError("generate_adaptive_pseudo_masks: adaptive is a dict of method, bins, floor, ceil")
    opts = dict(method="otsu", bins=256, floor=0.0, ceil=1.0)
    opts.update(adaptive)
    if opts["method"] != "otsu":
        raise ValueError(f"generate_adaptive_pseudo_masks: method {opts['method']!r}: 'otsu' is the one there is")
    if any(isinstance(opts[k], bool) or not isinstance(opts[k], (int, float)) for k in ("floor", "ceil")) or not opts["floor"] <= opts["ceil"]:
        raise ValueError(f"generate_adaptive_pseudo_masks: floor {opts['floor']!r} and ceil {opts['ceil']!r} must be numbers, floor <= ceil")
    ops.uniform_edges(0.0, 1.0, opts["bins"])                      # (refuses the bins it cannot have)
    return opts


def adaptive_masks(score_map, fallback, method="otsu", bins=256, floor=0.0, ceil=1.0):
    """uint8 masks of a score map (B,H,W) in [0, 1] cut at a threshold of its own per image: Otsu's threshold over ``bins`` uniform
    bins of [0, 1) (``ops.score_histogram`` + ``ops.otsu_threshold``; ``fallback`` for an image with fewer than two occupied bins),
    clamped to ``[floor, ceil]``, applied by ``ops.threshold_per_image(positive_only=True)``: ``v >= t and v > 0``.  No host read."""
    s = score_map.detach().float().contiguous()
    counts = ops.score_histogram(s, bins=bins, range=(0.0, 1.0))
    _k, t, _q = ops.otsu_threshold(counts, ops.uniform_edges(0.0, 1.0, bins, s.device), fallback=float(fallback))
    return ops.threshold_per_image(s, t.clamp(float(floor), float(ceil)), positive_only=True)


def generate_adaptive_pseudo_masks(loader, layercam_gen, adaptive, **kwargs):
    """``generate_pseudo_masks(loader, layercam_gen, **kwargs)`` with a threshold per image.  (A function of its own: the positional
    signature of ``generate_pseudo_masks`` is pinned.)  ``adaptive``: None (bit for bit ``generate_pseudo_masks``) or
    ``dict(method="otsu", bins=256, floor=0.0, ceil=1.0)`` - every ``>= cam_thresh`` of the pipeline, on the raw CAM as on the
    ``pamr`` / ``superpixels`` / ``affinity`` / ``boundary`` maps, becomes that map's own Otsu threshold per image
    (``adaptive_masks``), clamped to ``[floor, ceil]``; ``cam_thresh`` is the fallback for an image with fewer than two occupied
    bins; ``keep_largest`` follows as before.  The results are left where ``generate_pseudo_masks`` leaves them."""
    return _generate_pseudo_masks(loader, layercam_gen, adaptive=adaptive, **kwargs)


def generate_adaptive_prototype_pseudo_masks(loader, layercam_gen, prototype, adaptive, **kwargs):
    """``generate_prototype_pseudo_masks`` with the per-image threshold of ``generate_adaptive_pseudo_masks`` on the prototype CAM."""
    return _generate_pseudo_masks(loader, layercam_gen, prototype=prototype, adaptive=adaptive, **kwargs)


def _generate_pseudo_masks(loader, layercam_gen, cam_thresh=0.3, alpha=1.0, keep_largest_masks=True, run_id="default",
                           out_root="/content", max_images=500, write_png=True, device="cuda", rank=0, world=1, keep_images=False,
                           streams=3, keep_on_device=False, device_batch=0, pamr=None, superpixels=None, affinity=None, boundary=None,
                           multiscale=None, prototype=None, adaptive=None):
    """The body of ``generate_pseudo_masks`` / ``generate_prototype_pseudo_masks`` / ``generate_adaptive_pseudo_masks`` (their
    docstrings)."""
    if adaptive is not None:
        adaptive = _adaptive_options(adaptive)
    if prototype is not None:
        if pamr is not None or superpixels is not None or affinity is not None or boundary is not None:
            raise ValueError("generate_prototype_pseudo_masks: prototype cannot be combined with pamr=, superpixels=, affinity= or boundary=")
        prototype = _prototype_options(prototype)
    if multiscale is not None:
        if not isinstance(multiscale, dict) or set(multiscale) - {"scales", "flip", "reduce", "multiple"}:
            raise ValueError("generate_pseudo_masks: multiscale= is a dict of scales, flip, reduce, multiple")
        if device_batch > 0:
            raise ValueError("generate_pseudo_masks: multiscale= cannot be combined with device_batch > 0")
        if not hasattr(layercam_gen, "generate_multiscale"):
            raise ValueError("generate_pseudo_masks: multiscale= needs a generator with generate_multiscale")
    if boundary is not None:
        if pamr is not None or superpixels is not None or affinity is not None:
            raise ValueError("generate_pseudo_masks: boundary= cannot be combined with pamr=, superpixels= or affinity=")
        boundary = _boundary_options(boundary)
    if affinity is not None:
        if pamr is not None or superpixels is not None:
            raise ValueError("generate_pseudo_masks: affinity= cannot be combined with pamr= or superpixels=")
        affinity = _affinity_options(affinity)
    if superpixels is not None:
        if pamr is not None:
            raise ValueError("generate_pseudo_masks: superpixels= and pamr= cannot be combined")
        ops.check_slic_options(**dict(superpixels, name="generate_pseudo_masks: superpixels"))
    mask_dir = os.path.join(out_root, f"pseudo_masks_{run_id}")
    image_dir = os.path.join(out_root, f"images_{run_id}")
    if write_png:
        from PIL import Image
        for d in (mask_dir, image_dir):
            os.makedirs(d, exist_ok=True)
            if rank == 0:
                for f in os.listdir(d):
                    os.remove(os.path.join(d, f))
        if world > 1:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.barrier()                  # nobody writes before rank 0 has emptied the directories
    masks, ids, images, img_id = [], [], [], 0

    def finish(group):
        """CAM + threshold for the queued batches (``streams`` of them in flight), then the host part per image."""
        if not group:
            return
        # device_batch = 0 (the default): one launch sequence per loader batch - the masks depend on the loader's batches
        # only, not on ``streams``, on how batches are dealt to ranks or on what else was queued (bit-reproducible).
        # device_batch = n > 0 (throughput option, 0.135 instead of 0.182 ms/img at n = 32): the loader's batches are merged
        # into device batches of n images.  A merged batch has its own per-tensor amax scales, tile and K-split choices, so
        # its masks equal the per-batch ones only outside the fp32 band of the network (~4e-3 of the CAM's range) and DO
        # depend on the flush threshold and the sharding - not for runs that must be reproducible
        if multiscale is not None:
            outs = [layercam_gen.generate_multiscale(g[1], alpha=alpha, class_idx=g[2], thresh=cam_thresh, **multiscale) for g in group]
        elif hasattr(layercam_gen, "generate_coalesced"):
            outs = layercam_gen.generate_coalesced([g[1] for g in group], alpha, [g[2] for g in group], cam_thresh, streams, device_batch)
        elif hasattr(layercam_gen, "generate_batches"):
            outs = layercam_gen.generate_batches([g[1] for g in group], alpha, [g[2] for g in group], cam_thresh, streams)
        else:
            outs = [layercam_gen.generate_batch(g[1], alpha=alpha, class_idx=g[2], thresh=cam_thresh) for g in group]
        for (imgs, imgs_d, _l, first_id, take), (cam, m) in zip(group, outs):
            if adaptive is not None:                                 # the same maps, each cut at its own threshold per image
                if pamr is not None:
                    cam = ops.pamr(imgs_d, cam[:, None], **pamr)[:, 0]
                elif superpixels is not None:
                    cam = superpixel_cam(imgs_d, cam, **superpixels)
                elif affinity is not None:
                    cam = affinity_cam(imgs_d, cam, **affinity)
                elif boundary is not None:
                    cam = boundary_cam(imgs_d, cam, **boundary)
                elif prototype is not None:
                    cam = prototype_cam(imgs_d, cam, **prototype)
                m = adaptive_masks(cam, cam_thresh, **adaptive)
            elif pamr is not None:
                m = ops.pamr_labels(ops.pamr(imgs_d, cam[:, None], **pamr), thresh=cam_thresh).to(torch.uint8)
            elif superpixels is not None:
                m = (superpixel_cam(imgs_d, cam, **superpixels) >= cam_thresh).to(torch.uint8)
            elif affinity is not None:
                m = (affinity_cam(imgs_d, cam, **affinity) >= cam_thresh).to(torch.uint8)
            elif boundary is not None:
                m = (boundary_cam(imgs_d, cam, **boundary) >= cam_thresh).to(torch.uint8)
            elif prototype is not None:
                m = (prototype_cam(imgs_d, cam, **prototype) >= cam_thresh).to(torch.uint8)
            if keep_largest_masks:
                m = keep_largest_batched(m)
            m_host = m if keep_on_device and not write_png else m.cpu().numpy()
            for i in range(take):
                gid = first_id + i
                mi = m_host[i]
                masks.append(mi)
                ids.append(gid)
                if keep_images:
                    images.append(imgs[i].detach())
                if write_png:
                    mt = torch.from_numpy(mi).float().unsqueeze(0).expand(3, -1, -1)
                    Image.fromarray(_to_png_u8(mt)).save(os.path.join(mask_dir, f"{gid}.png"))
                    im = imgs[i].detach().cpu().clone()
                    im = (im - im.min()) / (im.max() - im.min())
                    Image.fromarray(_to_png_u8(im)).save(os.path.join(image_dir, f"{gid}.png"))

    group = []
    for j, (imgs, (labels, _)) in enumerate(loader):
        if img_id >= max_images:
            break
        take = min(imgs.size(0), max_images - img_id)          # PsuedoMasks.py:49 - the 500-image cap
        if j % world != rank:
            img_id += take
            continue
        imgs_d = _to_device_async(imgs[:take], device)
        labels_d = _to_device_async(torch.as_tensor(labels[:take]), device)
        group.append((imgs, imgs_d, labels_d, img_id, take))
        img_id += take
        queued = sum(g[4] for g in group)
        if (device_batch > 0 and queued >= device_batch * max(1, streams)) or (device_batch <= 0 and len(group) >= max(1, streams)):
            finish(group)
            group = []
    finish(group)
    generate_pseudo_masks.last_masks = masks
    generate_pseudo_masks.last_ids = ids
    generate_pseudo_masks.last_images = images
    return image_dir, mask_dir


generate = generate_pseudo_masks   # north-star alias "PsuedoMasks.generate"

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


_norm_cache = {}


def _norm_constants(device):
    """ImageNet mean / std on ``device``, made once: ``torch.tensor(..., device=...)`` is a copy from pageable host memory
    and makes the host wait for the stream - per call it put stage 1 -> stage 2 in lockstep with the device."""
    key = str(torch.device(device))
    if key not in _norm_cache:
        _norm_cache[key] = (torch.tensor(_MEAN, device=device).view(1, 3, 1, 1), torch.tensor(_STD, device=device).view(1, 3, 1, 1))
    return _norm_cache[key]


def nearest_resize_index(n_out, n_in, device):
    """PIL NEAREST source index: floor((i + 0.5) * n_in / n_out)."""
    return ((torch.arange(n_out, device=device, dtype=torch.float64) + 0.5) * (n_in / n_out)).floor().long().clamp_(max=n_in - 1)


@torch.no_grad()
def stage_handoff(images, masks, size=(256, 256), device="cuda", *, exact=False):
    """In-memory stage-1 -> stage-2 hand-off: what ``PseudoSegmentationDataset`` (SegmentationDataset.py:19-38) would
    read back from the PNGs ``generate_pseudo_masks`` writes (PsuedoMasks.py:68-74), without the file system.

    images (N,3,h,w) float (stage-1 inputs), masks (N,h,w) uint8 {0,1} ->
      images256 (N,3,H,W) float32 on ``device``: min-max rescale per image, 8-bit quantisation (save_image),
                bilinear resize (PIL BILINEAR up-sampling == align_corners=False; HIP kernel), /255, ImageNet normalise;
      masks256  (N,H,W) uint8 {0,255}: x255 (save_image of a 0/1 tensor), NEAREST resize.
    ``exact=True``: the 8-bit image goes through ``ops.pil_resize`` (Pillow's integer BILINEAR) instead of the float
    up-sampler: images256 then EQUALS the PNG round trip (the default is equal to one 8-bit level).
    """
    x = torch.as_tensor(images).to(device=device, dtype=torch.float32)
    lo = x.amin(dim=(1, 2, 3), keepdim=True)
    hi = x.amax(dim=(1, 2, 3), keepdim=True)
    q = ((x - lo) / (hi - lo)).mul(255).add(0.5).clamp(0, 255).floor()          # uint8 values, kept as float
    H, W = size
    if exact:
        # the 8-bit planes through Pillow's own fixed-point BILINEAR (ops.pil_resize: planar input = N * 3 one-channel
        # images), ToTensor + Normalize from a table: equal to the PNG round trip, not only to one 8-bit level
        from .SegmentationDataset import _normalize_table
        N, _, h, w = q.shape
        planes = q.to(torch.uint8).contiguous()
        desc = ops.pil_describe([(h, w)] * (3 * N), [i * h * w for i in range(3 * N)], (H, W), ops.PIL_BILINEAR, planes.device)
        u8, _ = ops.pil_resize(planes.view(-1), desc, 1, (H, W))
        table = _normalize_table().to(planes.device)
        img = torch.stack([table[c][u8.view(N, 3, H, W)[:, c].to(torch.int32)] for c in range(3)], dim=1)
        return img.contiguous(), _handoff_masks(masks, H, W, device)
    # PIL resamples 8-bit images in two passes - columns first, then rows - and rounds to 8 bits after each
    if q.shape[-1] != W:
        q = ops.bilinear_resize(q.contiguous(), (q.shape[-2], W)).add(0.5).floor().clamp(0, 255)
    if q.shape[-2] != H:
        q = ops.bilinear_resize(q.contiguous(), (H, W)).add(0.5).floor().clamp(0, 255)
    mean, std = _norm_constants(device)
    img = (q / 255.0 - mean) / std
    return img.contiguous(), _handoff_masks(masks, H, W, device)


def _handoff_masks(masks, H, W, device):
    if isinstance(masks, (list, tuple)) and len(masks) and torch.is_tensor(masks[0]):
        m = torch.stack(list(masks)).to(device)                        # device masks (keep_on_device): no host round trip
    else:
        m = torch.as_tensor(masks if torch.is_tensor(masks) else np.asarray(masks)).to(device)
    m = (m != 0).to(torch.uint8) * 255
    if tuple(m.shape[-2:]) != (H, W):
        ih = nearest_resize_index(H, m.shape[-2], device)
        iw = nearest_resize_index(W, m.shape[-1], device)
        m = m[:, ih][:, :, iw]
    return m.contiguous()
