"""The oracle of the integer SLIC superpixels and of the pooling over them (tests/slic_oracle.py) against independent
formulations - per-pixel loops for assignment and update, a sequential raster scan for the connectivity pass, ``np.add.at`` /
``np.bincount`` for the pooling - its properties, the option refusals of the new ops (raised before anything asks for a
device) and the declarations of the new entry points.  No device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in so.SHAPES if s[1] * s[2] <= 37 * 53]


# ------------------------------------------------------------------------------------------------ independent formulations
def loop_slic(img, S, m, num_iter):
    """(raw, centres) of one image with plain Python integers, pixel by pixel."""
    _, H, W = img.shape
    GH, GW = max(1, (H + S // 2) // S), max(1, (W + S // 2) // S)
    cen = []
    for gy in range(GH):
        for gx in range(GW):
            cy, cx = ((2 * gy + 1) * H) // (2 * GH), ((2 * gx + 1) * W) // (2 * GW)
            cen.append([16 * cy, 16 * cx] + [16 * int(img[j, cy, cx]) for j in range(3)])

    def assign_all():
        lab = np.zeros((H, W), dtype=np.int64)
        for y in range(H):
            for x in range(W):
                hy, hx = min(GH - 1, y * GH // H), min(GW - 1, x * GW // W)
                best = None
                for cy in range(hy - 1, hy + 2):
                    for cx in range(hx - 1, hx + 2):
                        if not (0 <= cy < GH and 0 <= cx < GW):
                            continue
                        k = cy * GW + cx
                        c = cen[k]
                        D = S * S * sum((16 * int(img[j, y, x]) - c[2 + j]) ** 2 for j in range(3)) \
                            + m * m * ((16 * y - c[0]) ** 2 + (16 * x - c[1]) ** 2)
                        if best is None or (D, k) < best:
                            best = (D, k)
                lab[y, x] = best[1]
        return lab

    lab = None
    for _ in range(num_iter):
        lab = assign_all()
        acc = [[0] * 6 for _ in cen]
        for y in range(H):
            for x in range(W):
                a = acc[lab[y, x]]
                a[0] += 1
                for j, v in enumerate((y, x, int(img[0, y, x]), int(img[1, y, x]), int(img[2, y, x]))):
                    a[1 + j] += v
        for k, a in enumerate(acc):
            if a[0]:
                cen[k] = [(16 * a[1 + j] + a[0] // 2) // a[0] for j in range(5)]
    if lab is None:
        lab = assign_all()
    return lab, np.array(cen, dtype=np.int64)


def scan_connectivity(raw, min_size):
    """The connectivity pass as a sequential raster scan: components by flood fill in raster order of their first pixels, every
    orphan handed to the component its left (upper) neighbour ENDS in, one component at a time."""
    H, W = raw.shape
    comp = -np.ones((H, W), dtype=np.int64)
    comps = []                                                              # (first pixel, label, pixels)
    for y in range(H):
        for x in range(W):
            if comp[y, x] >= 0:
                continue
            cid, stack, pix = len(comps), [(y, x)], []
            comp[y, x] = cid
            while stack:
                cy, cx = stack.pop()
                pix.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and comp[ny, nx] < 0 and raw[ny, nx] == raw[y, x]:
                        comp[ny, nx] = cid
                        stack.append((ny, nx))
            comps.append((y * W + x, int(raw[y, x]), pix))
    main = {}
    for cid, (first, lab, pix) in enumerate(comps):                         # ascending first pixel: a later equal area does not win
        if lab not in main or len(pix) > len(comps[main[lab]][2]):
            main[lab] = cid
    ends, rank, n = {}, {}, 0
    for cid, (first, lab, pix) in enumerate(comps):
        if main[lab] != cid and len(pix) < min_size and first != 0:
            y, x = divmod(first, W)
            nb = comp[y, x - 1] if x > 0 else comp[y - 1, x]
            assert nb < cid
            ends[cid] = ends[nb]                                            # the neighbour's chain has ended already
        else:
            ends[cid] = cid
            rank[cid] = n
            n += 1
    seg = np.zeros((H, W), dtype=np.int32)
    for cid, (_f, _l, pix) in enumerate(comps):
        for y, x in pix:
            seg[y, x] = rank[ends[cid]]
    return seg, n


def is_4_connected(mask):
    from scipy import ndimage
    return ndimage.label(mask, structure=so.FOUR)[1] == 1


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("content", ("noise", "blobs", "halves"))
def test_assignment_and_update_equal_the_per_pixel_loops(shape, content):
    B, H, W, step = shape
    images = so.make_batch(content, B, H, W, seed=2)
    for m, it in ((10, 3), (1, 1), (40, 0)):
        want = so.slic(images, step, m, it)
        for b in range(B):
            raw, cen = loop_slic(images[b], step, m, it)
            assert np.array_equal(want["raw"][b], raw) and np.array_equal(want["centres"][b], cen), (shape, content, m, it, b)


@pytest.mark.parametrize("content", ("noise", "checker", "blobs", "halves", "flat"))
def test_connectivity_equals_the_sequential_scan(content):
    for shape in ((2, 5, 7, 3), (1, 37, 53, 8), (1, 3, 300, 4), (1, 300, 3, 4), (1, 65, 130, 10)):
        B, H, W, step = shape
        images = so.make_batch(content, B, H, W, seed=4)
        for min_size in (1, None, 7, H * W + 1):
            want = so.slic(images, step, 10, 2, min_size)
            ms = so.default_min_size(step) if min_size is None else min_size
            for b in range(B):
                seg, n = scan_connectivity(want["raw"][b], ms)
                assert n == want["n_segments"][b] and np.array_equal(seg, want["segments"][b]), (shape, content, min_size, b)


def test_the_worst_cases_are_in_the_device_grid():
    """What the device cases must contain to mean anything: orphan chains of more than 100 components (noise), nearly every pixel
    an orphan (the checkerboard), a flat image that keeps all K labels, both paths of the assignment kernel."""
    cases = so.device_cases()
    assert {c[1] for c in cases} == set(so.SHAPES) and {c[0] for c in cases} == set(so.CONTENTS)
    assert {(c[2], c[3]) for c in cases} >= {(m, it) for m in so.COMPACTNESS for it in so.NUM_ITER}
    _, want, stats = so.case("noise", (2, 65, 130, 10))
    assert stats["chain"] > 100, stats
    _, want, stats = so.case("checker", (2, 65, 130, 10))
    assert stats["orphans"] > 0.95 * 2 * 65 * 130, stats
    _, want, stats = so.case("flat", (2, 65, 130, 10))
    assert stats["orphans"] == 0 and (want["n_segments"] == 7 * 13).all()   # a flat image keeps all K labels
    assert (1, 40, 70, 1) in so.SHAPES                                      # 66 x 18 cells around a tile: past the 512 kept on chip


@pytest.mark.parametrize("c", [c for c in so.device_cases() if c[1][1] * c[1][2] <= 65 * 130 and c[2:4] == (10, 10)],
                         ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-min{c[4]}")
def test_properties_of_the_segments(c):
    from weaklysuperviseddl_amd import ops
    content, shape, m, it, ms = c
    B, H, W, step = shape
    images, want, stats = so.case(*c)
    seg, n, raw = want["segments"], want["n_segments"], want["raw"]
    GH, GW = so.grid(H, W, step)
    assert seg.dtype == np.int32 and raw.min() >= 0 and raw.max() < GH * GW and want["centres"].shape == (images.shape[0], GH * GW, 5)
    assert ops.slic_max_segments(H, W, step, ms) == so.max_segments(H, W, step, ms) == GH * GW + H * W // (ms or so.default_min_size(step)) + 1
    for b in range(seg.shape[0]):
        assert n[b] <= ops.slic_max_segments(H, W, step, ms)
        ids, first = np.unique(seg[b].ravel(), return_index=True)
        assert np.array_equal(ids, np.arange(n[b]))                         # dense ...
        assert (np.diff(first) > 0).all()                                   # ... and ordered by first pixel
        for s in ids[:: max(1, len(ids) // 12)]:
            assert is_4_connected(seg[b] == s), (c, b, s)
        if ms == 1:                                                         # nothing is an orphan: raw's components as they are
            comp, _ = so.components4(raw[b])
            assert np.array_equal(np.unique(comp, return_inverse=True)[1].reshape(H, W), seg[b])
        if ms == H * W + 1:                                                 # everything but the main components and pixel 0's merges
            assert n[b] <= GH * GW + 1


# ------------------------------------------------------------------------------------------------ pooling
def test_superpixel_mean_against_add_at_and_float64():
    rng = np.random.default_rng(0)
    _, want, _ = so.case("different3", (2, 65, 130, 10))
    seg = want["segments"]
    B, H, W = seg.shape
    n_max = so.max_segments(H, W, 10)
    v = (rng.standard_normal((B, 3, H, W)) * 5).astype(np.float32)
    mean, count = so.superpixel_mean(v, seg, n_max)
    q = np.rint(v.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    for b in range(B):
        n = np.bincount(seg[b].ravel(), minlength=n_max)
        assert np.array_equal(count[b], n)
        for c in range(3):
            tot = np.zeros(n_max, dtype=np.int64)
            np.add.at(tot, seg[b].ravel(), q[b, c].ravel())
            ok = n > 0
            assert np.array_equal(mean[b, c][ok], (tot[ok] / (n[ok] * 2.0 ** 24)).astype(np.float32)) and not mean[b, c][~ok].any()
            exact = np.bincount(seg[b].ravel(), weights=v[b, c].ravel().astype(np.float64), minlength=n_max)[ok] / n[ok]
            # every q is within half a quantum (2^-25) of its value, and so is their mean; the result is rounded to float32 once
            assert (np.abs(mean[b, c][ok].astype(np.float64) - exact) <= 2.0 ** -24 + np.abs(exact) * 2.0 ** -24).all()
    snapped = so.superpixel_snap(v, seg, n_max)
    assert np.array_equal(snapped[1, 2], mean[1, 2][seg[1]])
    # clamping, NaN, empty ids, ids outside the buffer
    v2 = np.array([[[[1e9, -1e9, np.nan, 2.0, 4.0, 7.0]]]], dtype=np.float32)
    s2 = np.array([[[0, 1, 2, 3, 3, 9]]], dtype=np.int32)
    m2, c2 = so.superpixel_mean(v2, s2, 6)
    assert c2.tolist() == [[1, 1, 1, 2, 0, 0]]
    assert m2[0, 0, :2].tolist() == [32768.0, -32768.0] and np.isnan(m2[0, 0, 2]) and m2[0, 0, 3:].tolist() == [3.0, 0.0, 0.0]
    assert so.superpixel_snap(v2, s2, 6)[0, 0, 0, 3:].tolist() == [3.0, 3.0, 0.0]


def test_superpixel_vote_against_bincount():
    rng = np.random.default_rng(1)
    _, want, _ = so.case("noise", (2, 65, 130, 10))
    seg = want["segments"]
    B, H, W = seg.shape
    n_max = so.max_segments(H, W, 10)
    for NC in (2, 5):
        lab = rng.integers(-1, NC + 1, seg.shape)                           # -1 and NC are not counted
        got = so.superpixel_vote(lab, seg, n_max, NC, ignore_index=99)
        for b in range(B):
            for s in range(int(want["n_segments"][b])):
                m = seg[b] == s
                inside = lab[b][m][(lab[b][m] >= 0) & (lab[b][m] < NC)]
                expect = int(np.argmax(np.bincount(inside, minlength=NC))) if len(inside) else 99
                assert (got[b][m] == expect).all()
    tie = so.superpixel_vote(np.array([[[2, 1, 1, 2, 7, 7]]]), np.array([[[0, 0, 0, 0, 1, 1]]]), 3, 3)
    assert tie.tolist() == [[[1, 1, 1, 1, 255, 255]]]


# ------------------------------------------------------------------------------------------------ refusals, declarations
def test_option_refusals_need_no_device():
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks, refine_dataset
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    for kw in (dict(step=0), dict(step=129), dict(step=4.0), dict(step=True), dict(step=4, compactness=0), dict(step=4, compactness=256),
               dict(step=4, num_iter=-1), dict(step=4, num_iter=1.5), dict(step=4, min_size=0)):
        with pytest.raises(ValueError):
            ops.check_slic_options(**kw)
        with pytest.raises(ValueError):
            ops.slic(img, **kw)
        with pytest.raises(ValueError):
            wnn.Superpixels(**kw)
    assert ops.check_slic_options(16) == (16, 10, 10, 64) and ops.check_slic_options(1, 255, 0, 5) == (1, 255, 0, 5)
    assert ops.check_slic_options(128)[3] == 4096 and ops.check_slic_options(1)[3] == 1
    with pytest.raises(ValueError):
        ops.slic(img.float(), 4)                                            # float images go through slic_quantize
    with pytest.raises(ValueError):
        ops.slic(torch.zeros(1, 3, 8193, 2, dtype=torch.uint8), 4)
    with pytest.raises(ValueError):
        ops.check_slic_geometry(2, 1 << 15, 1 << 15)
    ops.check_slic_geometry(1, 8192, 8192)
    with pytest.raises(ops.WsdlError):
        ops.slic(img, 4)                                                    # a host tensor: there is no CPU fallback
    with pytest.raises(ops.WsdlError):
        ops.slic_quantize(img.float())
    assert ops.slic_max_segments(65, 130, 10) == 7 * 13 + 65 * 130 // 25 + 1 and ops.slic_max_segments(20, 30, 64, 1) == 1 + 600 + 1
    assert ops.slic_grid(20, 30, 64) == (1, 1) and ops.slic_grid(1, 7, 2) == (1, 4)
    assert ops.slic_launches(65, 130, 10) == 32 and ops.slic_launches(20, 30, 0) == 12 and ops.slic_launches(33, 64, 1) == 14
    seg, vals, lab = torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.superpixel_mean(vals, seg, bad)
        with pytest.raises(ValueError):
            ops.superpixel_vote(lab, seg, bad, 2)
    with pytest.raises(ValueError):
        ops.superpixel_snap(torch.zeros(1, 33, 8, 8), seg, 4)
    for bad in (0, 65, 2.0):
        with pytest.raises(ValueError):
            ops.superpixel_vote(lab, seg, 4, bad)
    with pytest.raises(ValueError):
        ops.superpixel_vote(lab, seg, 4, 2, ignore_index=0.5)
    with pytest.raises(ops.WsdlError):
        ops.superpixel_mean(vals, seg, 4)
    with pytest.raises(ops.WsdlError):
        ops.superpixel_vote(lab, seg, 4, 2)
    sp = wnn.Superpixels(16)
    assert (sp.step, sp.compactness, sp.num_iter, sp.min_size) == (16, 10, 10, 64) and "step=16" in repr(sp)
    assert not list(sp.parameters())
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, superpixels={"step": 8}, pamr={})
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, superpixels={"step": 0})
    with pytest.raises(ValueError):
        refine_dataset(None, [], method="superpixel", superpixel_kwargs={"step": 300})
    with pytest.raises(ValueError):
        refine_dataset(None, [], method="slic")


def test_callers_keep_their_defaults():
    import inspect
    from weaklysuperviseddl_amd.TraditionalModel import refine_dataset, generate_pseudo_masks
    p = inspect.signature(refine_dataset).parameters
    assert p["method"].default == "ncut" and p["superpixel_kwargs"].default is None and p["pamr_kwargs"].default is None
    assert inspect.signature(generate_pseudo_masks).parameters["superpixels"].default is None


def test_the_new_entry_points_are_declared_bound_and_exported():
    from weaklysuperviseddl_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    names = ("wsdl_slic", "wsdl_slic_workspace", "wsdl_superpixel_mean", "wsdl_superpixel_vote", "wsdl_superpixel_workspace")
    for name in names:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    for name in names[:4]:
        assert re.search(r"%s: no counterpart in the reference" % name, header) or name == "wsdl_slic_workspace", name
    assert "slic.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "slic.hip"))
    assert os.path.exists(os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "components_grid.h"))
    handle = ctypes.CDLL(_lib.LIB_PATH)                                     # the built library exports them (no device needed)
    for name in names:
        assert hasattr(handle, name), name
    # the geometry refusals of the library need no device either
    q = handle.wsdl_slic_workspace
    q.restype, q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    assert q(1, 8, 8, 4) > 0 and q(1, 8, 8, 0) == 0 and q(1, 8, 8, 129) == 0 and q(1, 8193, 8, 4) == 0 and q(0, 8, 8, 4) == 0
    assert q(2, 1 << 13, 1 << 13, 16) > 0
