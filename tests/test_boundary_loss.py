"""The oracle of tests/boundary_loss_oracle.py against independent formulations on the CPU - the published scipy formula of the
signed distance map, torch autograd of ``einsum`` + ``mean`` in float64, ``binary_erosion`` surfaces and scipy's transform of
the surface map - the nearest-rank rule against the rank rule of ``kth_value``, the host arithmetic of
``ops.surface_distances_from_stats`` and every option check that needs no device."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_loss_oracle as bo  # noqa: E402
import edt_oracle as eo  # noqa: E402
import pixel_mining_oracle as pmo  # noqa: E402

SCIPY_CASES = [c for c in bo.CASES if c[1] * c[2] >= 64 and c[1] * c[2] <= 5000]


# ------------------------------------------------------------------------------------------------------ signed distance
@pytest.mark.parametrize("case", range(len(SCIPY_CASES)))
def test_phi_equals_the_published_scipy_formula(case):
    """one_hot2dist of the paper's code: distance(negmask) * negmask - (distance(posmask) - 1) * posmask."""
    ndi = pytest.importorskip("scipy.ndimage")
    B, H, W = SCIPY_CASES[case]
    labels = eo.make_labels(B, H, W, 500 + case)
    for value in (1, 0):
        phi = bo.signed_distance(labels, value)
        pos = (labels == value).numpy()
        for b in range(B):
            assert pos[b].any() and not pos[b].all()                    # (scipy needs a pixel of each kind)
            neg = ~pos[b]
            want = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos[b]) - 1) * pos[b]
            assert np.allclose(phi[b].numpy(), want, rtol=1e-15, atol=0), (value, b)
        assert (phi[labels == value] <= 0).all() and (phi[labels != value] >= 1).all()


@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_axis_by_axis_planes_equal_the_all_pairs_oracle(case):
    """Up to 64 x 64 against ``eo.dist2``; at 96 x 130, where that takes seconds per plane, against scipy."""
    B, H, W = bo.CASES[case]
    labels = eo.make_labels(B, H, W, 700 + case)
    for value in (1, 0, 2, 7):
        got = bo.dist2_separable(labels, value)
        if H * W <= 4096:
            want = eo.dist2(labels, value, "euclid", False)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), value
        elif value != 7:
            ndi = pytest.importorskip("scipy.ndimage")
            inside = (labels == value).numpy()
            for b in range(B):
                assert inside[b].any() and not inside[b].all()
                assert np.array_equal(got[0][b].numpy(), np.round(ndi.distance_transform_edt(inside[b]) ** 2).astype(np.int64))
                assert np.array_equal(got[1][b].numpy(), np.round(ndi.distance_transform_edt(~inside[b]) ** 2).astype(np.int64))
        else:
            assert (got[0] == 0).all() and (got[1] == bo.FAR).all()      # an absent class


def test_phi_of_absent_and_full_classes_and_void_pixels():
    labels = eo.make_labels(3, 9, 11, 7)
    labels[1] = 1                                                        # the class fills the image
    labels[2][labels[2] == 1] = 0                                        # the class is absent
    phi = bo.signed_distance(labels, 1)
    assert (phi[1] == 0).all() and (phi[2] == 0).all() and (phi[0] != 0).any()
    assert (labels[0] == 255).any() and (phi[0][labels[0] == 255] >= 1).all()          # void pixels are OUT
    stacked = bo.signed_distance_classes(labels, (2, 0), torch.float32)
    assert stacked.dtype == torch.float32 and tuple(stacked.shape) == (3, 2, 9, 11)
    assert torch.equal(stacked[:, 1], bo.signed_distance(labels, 0, torch.float32))


# ------------------------------------------------------------------------------------------------------ loss and gradient
@pytest.mark.parametrize("C,classes,ignore", ((2, (1,), None), (3, (0, 1), 255), (3, (2, 0), 255), (21, (2, 0), 255)))
def test_loss_and_gradient_equal_autograd_of_einsum_and_mean(C, classes, ignore):
    B, H, W = 2, 9, 11
    labels = eo.make_labels(B, H, W, 11)
    phi = bo.signed_distance_classes(labels, classes)
    z = bo.make_logits(B, C, H, W, 3).double().requires_grad_()
    s = torch.softmax(z, dim=1)[:, list(classes)]
    if ignore is None:
        ref = torch.einsum("bkhw,bkhw->bkhw", s, phi).mean()
        got, grad = bo.loss_and_grad(z.detach(), phi, None, classes)
    else:
        valid = labels != ignore
        assert 0 < int(valid.sum()) < valid.numel()
        ref = torch.einsum("bkhw,bkhw->bhw", s, phi)[valid].sum() / (len(classes) * int(valid.sum()))
        got, grad = bo.loss_and_grad(z.detach(), phi, labels, classes, ignore)
    ref.backward()
    assert abs(float(got) - ref.item()) <= 1e-14 * max(1.0, abs(ref.item()))
    assert (grad - z.grad).abs().max().item() <= 1e-15
    if ignore is not None:
        assert (grad.permute(0, 2, 3, 1)[labels == ignore] == 0).all()
    l2, g2 = bo.loss_and_grad(z.detach(), phi, labels, classes, -100 if ignore is None else ignore, scale=0.37)
    assert abs(float(l2) - 0.37 * float(got)) <= 1e-15 and (g2 - 0.37 * grad).abs().max().item() <= 1e-16
    l0, g0 = bo.loss_and_grad(z.detach(), phi, torch.full_like(labels, 255), classes, 255)
    assert float(l0) == 0.0 and not g0.any()
    l32, g32 = bo.loss_and_grad(z.detach().float(), phi.float(), labels, classes, -100 if ignore is None else ignore, dtype=torch.float32)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32 and abs(float(l32) - float(got)) < 1e-4


# ------------------------------------------------------------------------------------------------------ surfaces
@pytest.mark.parametrize("case", range(len(SCIPY_CASES)))
def test_surfaces_and_directed_distances_equal_scipy(case):
    ndi = pytest.importorskip("scipy.ndimage")
    B, H, W = SCIPY_CASES[case]
    a = eo.make_labels(B, H, W, 600 + case) == 1
    b = torch.roll(a, (1, -2), (1, 2))
    b[0, :, 0] = True                                                    # touches the image edge
    sa, sb = bo.surface(a), bo.surface(b)
    for m, s in ((a, sa), (b, sb)):
        for i in range(B):
            mm = m[i].numpy()
            assert np.array_equal(s[i].numpy(), mm ^ ndi.binary_erosion(mm, border_value=0))
    assert sb[0, :, 0].all()
    for s_from, s_to in ((sa, sb), (sb, sa)):
        got = bo.directed_d2(s_from, s_to)
        for i in range(B):
            want = ndi.distance_transform_edt(~s_to[i].numpy())[s_from[i].numpy()]
            assert np.array_equal(got[i].numpy(), np.round(want ** 2).astype(np.int64))
    # a border=True transform finds the same surface: IN pixels at squared distance 1 from the outside
    d_out, _ = eo.dist2(a, 1, "euclid", True)
    assert torch.equal(sa, d_out == 1)


def test_stats_and_metrics_on_hand_made_masks():
    """8 x 8: G = rows 2..5 x cols 2..5, P = the same square two columns to the right.  Both surfaces are rings of 12.  Every
    ring pixel of P in columns 6, 7 is 1 or 2 from G's ring column 5; the Hausdorff distance is 2 (P's column 7 to G's column
    5 and G's column 2 to P's column 4)."""
    g = torch.zeros(4, 8, 8, dtype=torch.int64)
    p = torch.zeros(4, 8, 8, dtype=torch.int64)
    g[0, 2:6, 2:6] = 1
    p[0, 2:6, 4:8] = 1
    g[1, 2:6, 2:6] = 1
    p[1] = g[1]                                                          # identical
    g[2, 3, 3] = 1                                                       # an empty prediction
    p[3, 0, 0] = 1                                                       # one pixel each, in opposite corners
    g[3, 7, 7] = 1
    st = bo.surface_stats(p, g)
    assert st["n"].tolist() == [[12, 12], [12, 12], [0, 1], [1, 1]]
    assert st["max_d2"].tolist() == [[4, 4], [0, 0], [0, bo.FAR], [98, 98]]
    assert st["pct_d2"][2, 0] == math.inf and st["pct_d2"][3].tolist() == [98.0, 98.0]
    per, means, defined = bo.metrics(st)
    assert defined == 3 and per[0]["hd"] == 2.0 and per[1] == {"hd": 0.0, "hd95": 0.0, "assd": 0.0}
    assert math.isnan(per[2]["hd"]) and per[3]["hd"] == math.sqrt(98.0) == per[3]["assd"]
    assert means["hd"] == (2.0 + 0.0 + math.sqrt(98.0)) / 3


# ------------------------------------------------------------------------------------------------------ nearest rank
@pytest.mark.parametrize("n", (1, 7, 19, 20, 21, 40, 100, 1961))
@pytest.mark.parametrize("percentile", (95.0, 50.0, 100.0, 99.5))
def test_nearest_rank_restates_the_rank_rule_of_kth_value(n, percentile):
    """wsdl_kth_value selects the min(n, k + floor(frac n))-th largest (tests/pixel_mining_oracle.py ``rank``); with k = 1 and
    frac = 1 - p / 100 that is the nearest-rank percentile - the ceil(p n / 100)-th smallest - whenever (1 - p / 100) n is
    not within rounding of an integer from below; at n a multiple of 20 and p = 95 the double product lands just ABOVE the
    integer (0.05 is stored as 0.05000000000000004), which keeps the rule."""
    frac = 1.0 - percentile / 100.0
    K = bo.rank(n, percentile)
    assert K == pmo.rank(n, 1, frac) and 1 <= K <= n
    from fractions import Fraction
    exact = Fraction(percentile).limit_denominator(1000) * n / 100
    assert n - K + 1 == max(1, math.ceil(exact)), (n, percentile, K)        # K-th largest == ceil(p n / 100)-th smallest
    g = torch.Generator().manual_seed(n)
    d2 = torch.randint(0, 50, (n,), generator=g)
    value, cnt = pmo.kth_value_exact(d2.float().numpy(), 1, frac, True)
    assert cnt == n and float(value) == bo.nearest_rank(d2, percentile)
    if percentile == 100.0:
        assert bo.nearest_rank(d2, percentile) == float(d2.max())
    assert bo.nearest_rank(d2[:0], percentile) == math.inf


# ------------------------------------------------------------------------------------------------------ host arithmetic
def test_surface_distances_from_stats_handles_nan_images():
    from weaklysuperviseddl_amd import ops
    g = torch.zeros(3, 8, 8, dtype=torch.int64)
    p = torch.zeros(3, 8, 8, dtype=torch.int64)
    g[0, 2:6, 2:6] = 1
    p[0, 2:6, 4:8] = 1
    g[1, 3, 3] = 1
    g[2, 1:4, 1:7] = 1
    p[2, 2:7, 0:5] = 1
    st = bo.surface_stats(p, g)
    per, means, defined = ops.surface_distances_from_stats(st)
    want_per, want_means, want_defined = bo.metrics(st)
    assert defined == want_defined == 2 and means == want_means
    assert math.isnan(per[1]["hd"]) and math.isnan(per[1]["hd95"]) and math.isnan(per[1]["assd"])
    assert per[0] == want_per[0] and per[2] == want_per[2]
    # the all-nan case
    empty = {k: v[1:2] for k, v in st.items()}
    per, means, defined = ops.surface_distances_from_stats(empty)
    assert defined == 0 and all(math.isnan(v) for v in means.values()) and len(per) == 1
    # the packed rows are a lossless detour
    rows = np.concatenate([st[k].astype(np.float64) for k in ("n", "max_d2", "sum_d", "pct_d2")], axis=1)
    back = ops.surface_stats_from_rows(rows)
    assert all(np.array_equal(back[k], st[k]) for k in st)
    with pytest.raises(ValueError):
        ops.surface_distances_from_stats({k: v[:0] for k, v in st.items()})


# ------------------------------------------------------------------------------------------------------ option checks
def test_option_checks_need_no_device():
    from weaklysuperviseddl_amd import ops, plan, nn as wnn
    for bad in ((), (1, 1), (-1,), (1.0,), (True,), 1, tuple(range(33)), "1"):
        with pytest.raises(ValueError):
            ops.check_boundary_classes(bad)
        with pytest.raises(ValueError):
            wnn.BoundaryLoss(classes=bad)
        with pytest.raises(ValueError):
            wnn.CrossEntropyBoundaryLoss(classes=bad)
    assert ops.check_boundary_classes([2, 0]) == (2, 0) and ops.check_boundary_classes(tuple(range(32))) == tuple(range(32))
    z = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError):
        ops.boundary_loss(z, torch.zeros(1, 1, 4, 4), classes=(2,))       # a class outside [0, C)
    with pytest.raises(ValueError):
        ops.signed_distance_classes(torch.zeros(1, 4, 4, dtype=torch.int64), ())
    with pytest.raises(ValueError):
        ops.signed_distance(torch.zeros(1, 4, 4, dtype=torch.int64), 1.5)
    for bad in (0.0, -5.0, 100.5, True, "95"):
        with pytest.raises(ValueError):
            ops.check_percentile(bad)
        with pytest.raises(ValueError):
            ops.surface_distance_stats(torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 4, dtype=torch.int64), percentile=bad)
    for bad in (-0.1, float("inf"), float("nan"), True, None):
        with pytest.raises(ValueError):
            wnn.CrossEntropyBoundaryLoss(alpha=bad)
    with pytest.raises(ValueError):
        wnn.CrossEntropyBoundaryLoss(label_smoothing=1.5)
    with pytest.raises(ValueError):
        wnn.CrossEntropyBoundaryLoss(weight=torch.zeros(2, 2))
    # no CPU fallback
    with pytest.raises(ops.WsdlError):
        ops.boundary_loss(z, torch.zeros(1, 1, 4, 4))
    with pytest.raises(ops.WsdlError):
        ops.signed_distance(torch.zeros(1, 4, 4, dtype=torch.int64))
    # the plan key: classes and ignore_index are in it, alpha is not (it lives on the device)
    def key(obj):
        """host_scalars without the addresses (two objects never share a buffer)."""
        def strip(t):
            if isinstance(t, tuple):
                if len(t) == 2 and isinstance(t[0], str) and t[0].endswith("_ptr"):
                    return None
                return tuple(strip(v) for v in t)
            return t
        return strip(plan.host_scalars(obj))

    base = key(wnn.CrossEntropyBoundaryLoss())
    assert base == key(wnn.CrossEntropyBoundaryLoss(alpha=0.5)) and "classes_key" in str(base) and "alpha_dev_ptr" not in str(base)
    for kw in (dict(classes=(0,)), dict(classes=(1, 0)), dict(ignore_index=255), dict(label_smoothing=0.1)):
        assert key(wnn.CrossEntropyBoundaryLoss(**kw)) != base, kw
    assert key(wnn.BoundaryLoss()) != key(wnn.BoundaryLoss(classes=(0,)))
    crit = wnn.CrossEntropyBoundaryLoss(alpha=0.25)
    full = plan.host_scalars(crit)
    assert "alpha_dev_ptr" in str(full)
    ptr = crit.alpha_dev.data_ptr()
    assert crit.set_alpha(0.5) is crit and crit.alpha_dev.item() == 0.5 and crit.alpha_dev.data_ptr() == ptr
    assert plan.host_scalars(crit) == full
    crit.boundary.set_classes((0,))
    assert plan.host_scalars(crit) != full
    with pytest.raises(ValueError):
        crit.set_alpha(-1.0)


def test_exports_and_signatures():
    import inspect
    from weaklysuperviseddl_amd import ops, _lib
    from weaklysuperviseddl_amd import TraditionalModel as tm
    for name in ("wsdl_signed_distance", "wsdl_boundary_loss_fwd_bwd", "wsdl_surface_map", "wsdl_surface_stats",
                 "wsdl_surface_stats_workspace"):
        assert name in _lib.SIGNATURES
    assert callable(tm.evaluate_surface_distances)
    sig = inspect.signature(ops.boundary_loss)
    assert [p for p, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["classes", "ignore_index", "scale"]
    assert inspect.signature(ops.surface_distance_stats).parameters["percentile"].default == 95.0
    assert _lib.lib().wsdl_surface_stats_workspace(3) > 0 and _lib.lib().wsdl_surface_stats_workspace(0) == 0
