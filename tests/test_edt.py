"""The brute-force oracle of tests/edt_oracle.py against independent formulations on the CPU (scipy's distance transforms,
iterated erosion), hand-made Boundary IoU values, the sentinel rules and the ABI table.  No device needed.

Hand-made 8 x 8 cases of Boundary IoU (width 1 unless stated; the boundary region of an a x a square, a >= 2, at width 1 is
its outer ring of 4a - 4 pixels, also where the square touches the image edge, which counts as background):
  A  G = rows 2..5 x cols 2..5, P = the same square one column to the right.  Both rings have 12 pixels.  They share
     columns 3, 4, 5 of rows 2 and 5 (in rows 3, 4 G's ring holds columns 2, 5 and P's 3, 6): 6 pixels; union 18; IoU = 1/3.
  B  P = G: IoU = 1.
  C  both empty: the union is empty, IoU = EMPTY = 1.
  D  G = rows 0..3 x cols 0..3 (a corner: ring of 12), P = the whole image (ring of 28).  They share row 0, columns 0..3 and
     column 0, rows 1..3: 7 pixels; union 12 + 28 - 7 = 33; IoU = 7/33.
  E  width 3, G = rows 3..4 x cols 3..4, P = one column to the right: a band wider than the object is the object, 4 pixels
     each, sharing column 4: 2 pixels; union 6; IoU = 1/3.
The batch (A, B, C, D) has the mean (1/3 + 1 + 1 + 7/33) / 4."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_oracle as eo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCIPY_CASES = [c for c in eo.CASES if c[1] * c[2] >= 64]


def square(r0, r1, c0, c1):
    m = torch.zeros(8, 8, dtype=torch.int64)
    m[r0:r1 + 1, c0:c1 + 1] = 1
    return m


def hand_cases():
    g = torch.stack([square(2, 5, 2, 5), square(2, 5, 2, 5), torch.zeros(8, 8, dtype=torch.int64), square(0, 3, 0, 3)])
    p = torch.stack([square(2, 5, 3, 6), square(2, 5, 2, 5), torch.zeros(8, 8, dtype=torch.int64), square(0, 7, 0, 7)])
    return p, g, [(6, 18), (12, 12), (0, 0), (7, 33)]


@pytest.mark.parametrize("case", range(len(SCIPY_CASES)))
def test_oracle_equals_scipy_for_both_metrics_and_polarities(case):
    ndi = pytest.importorskip("scipy.ndimage")
    B, H, W = SCIPY_CASES[case]
    labels = eo.make_labels(B, H, W, 100 + case)
    inside = (labels == 1).numpy()
    assert inside.any() and not inside.all()
    for metric in eo.METRICS:
        d_out, d_in = eo.dist2(labels, 1, metric)
        for b in range(B):
            if metric == "euclid":
                want_out = ndi.distance_transform_edt(inside[b]) ** 2
                want_in = ndi.distance_transform_edt(~inside[b]) ** 2
            else:
                want_out = ndi.distance_transform_cdt(inside[b], metric="chessboard").astype("int64") ** 2
                want_in = ndi.distance_transform_cdt(~inside[b], metric="chessboard").astype("int64") ** 2
            assert inside[b].any() and not inside[b].all()          # (scipy needs a site of each kind)
            assert torch.equal(d_out[b], torch.from_numpy(want_out).round().long()), (metric, b)
            assert torch.equal(d_in[b], torch.from_numpy(want_in).round().long()), (metric, b)
        assert (d_out[labels != 1] == 0).all() and (d_in[labels == 1] == 0).all()
        assert (d_out[labels == 1] > 0).all() and (d_in[labels != 1] > 0).all()


@pytest.mark.parametrize("case", range(len(SCIPY_CASES)))
def test_padded_border_equals_scipy_on_the_padded_image(case):
    ndi = pytest.importorskip("scipy.ndimage")
    import numpy as np
    B, H, W = SCIPY_CASES[case]
    labels = eo.make_labels(B, H, W, 100 + case)
    inside = (labels == 1).numpy()
    for metric in eo.METRICS:
        d_out, d_in = eo.dist2(labels, 1, metric, border=True)
        assert torch.equal(d_in, eo.dist2(labels, 1, metric)[1])            # the border does not reach d2_in
        for b in range(B):
            padded = np.pad(inside[b], max(H, W) + 1)                       # more rings than any walk needs
            if metric == "euclid":
                want = ndi.distance_transform_edt(padded) ** 2
            else:
                want = ndi.distance_transform_cdt(padded, metric="chessboard").astype("int64") ** 2
            p = max(H, W) + 1
            assert torch.equal(d_out[b], torch.from_numpy(want[p:p + H, p:p + W]).round().long()), (metric, b)


@pytest.mark.parametrize("case", range(len(eo.CASES)))
def test_erosion_band_equals_the_distance_band(case):
    B, H, W = eo.CASES[case]
    for value in (1, 2):
        labels = eo.make_labels(B, H, W, 200 + case)
        d_out, _ = eo.dist2(labels, value, "chebyshev", border=True)
        for width in (1, 2, 3, 7):
            assert torch.equal(eo.band(labels == value, width), (d_out > 0) & (d_out <= width * width)), (value, width)


def test_boundary_iou_on_hand_made_cases():
    p, g, want = hand_cases()
    assert eo.boundary_iou_counts(p, g, 1) == want
    assert eo.boundary_iou_counts(g, p, 1) == want                         # symmetric
    assert eo.boundary_iou(p[:1], g[:1], width=1) == 1.0 / 3.0
    assert eo.boundary_iou(p[3:], g[3:], width=1) == 7.0 / 33.0
    assert eo.boundary_iou(p, g, width=1) == (1.0 / 3.0 + 1.0 + 1.0 + 7.0 / 33.0) / 4
    assert eo.mean_iou([(0, 0)], EMPTY=0.0) == 0.0
    # E: a band wider than the object is the object
    ge, pe = square(3, 4, 3, 4)[None], square(3, 4, 4, 5)[None]
    assert eo.boundary_iou_counts(pe, ge, 3) == [(2, 6)] and torch.equal(eo.band(ge == 1, 3), ge == 1)
    # the published width: 2 % of the diagonal, at least one pixel
    assert eo.boundary_width(8, 8) == 1 and eo.boundary_width(224, 224) == 6 and eo.boundary_width(37, 53, 0.1) == 6


def test_host_arithmetic_of_the_package_equals_the_oracle():
    from weaklysuperviseddl_amd import ops
    _, _, want = hand_cases()
    assert ops.boundary_iou_from_counts(want) == eo.mean_iou(want) == (1.0 / 3.0 + 1.0 + 1.0 + 7.0 / 33.0) / 4
    assert ops.boundary_iou_from_counts(torch.tensor(want).numpy(), EMPTY=0.0) == eo.mean_iou(want, EMPTY=0.0)
    assert ops.boundary_iou_from_counts([(7, 33)]) == 7.0 / 33.0
    for hw in ((8, 8), (224, 224), (37, 53), (1, 1), (500, 375)):
        for ratio in (0.02, 0.1):
            assert ops.boundary_width(*hw, ratio) == eo.boundary_width(*hw, ratio)
    assert ops.EDT_FAR == eo.FAR
    with pytest.raises(ValueError):
        ops.check_boundary_confidence_options(0.0, 0.0)
    with pytest.raises(ValueError):
        ops.check_boundary_confidence_options(3.0, 1.5)
    with pytest.raises(ValueError):
        ops.edt(torch.zeros(1, 2, 2, dtype=torch.int64), metric="manhattan")
    with pytest.raises(ops.WsdlError):
        ops.edt(torch.zeros(1, 2, 2, dtype=torch.int64))                   # a host tensor: no CPU fallback


def test_sentinel_rules():
    ones = torch.ones(1, 4, 5, dtype=torch.int64)
    for metric in eo.METRICS:
        d_out, d_in = eo.dist2(ones, 1, metric)
        assert (d_out == eo.FAR).all() and (d_in == 0).all()               # all IN, no border: no OUT pixel anywhere
        d_out, d_in = eo.dist2(ones, 1, metric, border=True)
        want = torch.minimum(torch.minimum(torch.arange(1, 5)[:, None], torch.arange(4, 0, -1)[:, None]),
                             torch.minimum(torch.arange(1, 6)[None], torch.arange(5, 0, -1)[None])) ** 2
        assert torch.equal(d_out[0], want)                                  # column x is x + 1 from the outside
        d_out, d_in = eo.dist2(ones, 2, metric, border=True)
        assert (d_out == 0).all() and (d_in == eo.FAR).all()               # no IN pixel: the border does not reach d2_in
    # every true squared distance at the largest supported size stays below 2^28
    assert 2 * 8191 ** 2 < 1 << 28 < eo.FAR
    w = eo.confidence(*eo.dist2(ones, 1), sigma=2.0, floor=0.25)
    assert torch.equal(w, torch.ones_like(w))                               # no boundary: full confidence
    lab = torch.tensor([[[0, 1, 1, 1]]])
    w = eo.confidence(*eo.dist2(lab, 1), sigma=3.0, floor=0.25)
    e1, e4 = 0.25 + 0.75 * (1 - torch.exp(torch.tensor(-1 / 18.0, dtype=torch.float64))), 0.25 + 0.75 * (1 - torch.exp(torch.tensor(-4 / 18.0, dtype=torch.float64)))
    assert torch.allclose(w.flatten(), torch.stack([e1, e1, e4, 0.25 + 0.75 * (1 - torch.exp(torch.tensor(-9 / 18.0, dtype=torch.float64)))]), rtol=0, atol=1e-15)
    assert torch.equal(eo.confidence(*eo.dist2(lab, 1), sigma=3.0, floor=1.0), torch.ones(1, 1, 4, dtype=torch.float64))


def test_signatures_and_header_hold_the_three_symbols():
    from weaklysuperviseddl_amd import _lib
    header = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("wsdl_edt", "wsdl_band_counts", "wsdl_boundary_confidence"):
        assert name in _lib.SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert re.search(r"#define\s+WSDL_EDT_FAR\s+\(1\s*<<\s*30\)", code)
    lib = _lib.lib()
    # geometry is validated on the host: refused without touching a device
    for H, W, B in ((0, 4, 1), (4, 0, 1), (8193, 4, 1), (4, 8193, 1), (4, 4, 0), (8192, 8192, 32)):
        assert lib.wsdl_edt(None, 1, B, H, W, 0, 0, None, None, None) == -1, (H, W, B)
        assert b"edt" in lib.wsdl_last_error()
    assert lib.wsdl_edt(None, 1, 1, 4, 4, 2, 0, None, None, None) == -1     # an unknown metric
    assert lib.wsdl_band_counts(None, None, 1, 1, 16, None, None) == -1
    assert lib.wsdl_boundary_confidence(None, None, 3.0, 0.0, None, 16, None) == -1
