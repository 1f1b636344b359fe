"""The weighted cross entropy without a device: the float64 oracle (tests/weighted_ce_oracle.py) against live torch, the
criterion mapping, the argument checks and the plan keys of ``wnn.CrossEntropyLoss``."""
import inspect
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from weighted_ce_oracle import weighted_ce  # noqa: E402

BOUND = 1e-12


def _case(C, ignore_index, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, C, 5, 7, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, C, (2, 5, 7), generator=g)
    y[torch.rand(2, 5, 7, generator=g) < 0.2] = ignore_index
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.25
    p = torch.rand(2, 5, 7, generator=g, dtype=torch.float64)
    p[torch.rand(2, 5, 7, generator=g) < 0.2] = 0.0
    return z, y, w, p


def _err(a, b):
    """max |a - b|, relative to max |b| where that exceeds 1 (C = 1 has an exactly zero gradient in torch and rounding of
    the order 1e-19 in the closed form: a purely relative figure would mean nothing there)."""
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


GRID = list(itertools.product((1, 2, 3, 21), (0.0, 0.1, 1.0), (False, True), ("mean", "sum", "none"), (-100, 255)))


@pytest.mark.parametrize("C,eps,weighted,reduction,ignore_index", GRID)
def test_oracle_equals_torch_cross_entropy_in_float64(C, eps, weighted, reduction, ignore_index):
    z, y, w, _ = _case(C, ignore_index, 100 * C + (ignore_index == 255))
    weight = w if weighted else None
    zt = z.clone().requires_grad_(True)
    ref = F.cross_entropy(zt, y, weight=weight, ignore_index=ignore_index, reduction=reduction, label_smoothing=eps)
    g = torch.Generator().manual_seed(7)
    up = torch.rand(ref.shape, generator=g, dtype=torch.float64) + 0.5
    ref.backward(up)
    loss, grad = weighted_ce(z, y, ignore_index, weight, eps, reduction, upstream=up)
    assert loss.shape == ref.shape
    assert _err(loss, ref.detach()) <= BOUND
    assert _err(grad, zt.grad) <= BOUND


@pytest.mark.parametrize("C,eps,weighted,reduction", list(itertools.product((2, 21), (0.0, 0.1), (False, True),
                                                                              ("mean", "sum", "none"))))
def test_oracle_with_pixel_weights_equals_the_weighted_torch_map(C, eps, weighted, reduction):
    z, y, w, p = _case(C, -100, 31 + C)
    weight = w if weighted else None
    zt = z.clone().requires_grad_(True)
    pix = F.cross_entropy(zt, y, weight=weight, reduction="none", label_smoothing=eps) * p
    if reduction == "none":
        ref = pix
    elif reduction == "sum":
        ref = pix.sum()
    else:       # the quotient: the pixel-weighted sum over the pixel-weighted weights of the target classes
        wy = (w if weighted else torch.ones(C, dtype=torch.float64))[y.clamp_min(0)] * (y != -100)
        ref = pix.sum() / (p * wy).sum()
    up = torch.rand(ref.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 0.5
    ref.backward(up)
    loss, grad = weighted_ce(z, y, -100, weight, eps, reduction, pixel_weight=p, upstream=up)
    assert _err(loss, ref.detach()) <= BOUND
    assert _err(grad, zt.grad) <= BOUND
    # a zero pixel weight is an ignored pixel
    y2 = torch.where(p == 0, torch.full_like(y, -100), y)
    loss2, grad2 = weighted_ce(z, y2, -100, weight, eps, reduction, pixel_weight=torch.where(p == 0, torch.ones_like(p), p),
                               upstream=up)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_resolve_criterion_maps_class_weights_and_sum_onto_the_kernel():
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import resolve_criterion
    assert callable(resolve_criterion(torch.nn.CrossEntropyLoss(weight=torch.ones(2))))
    assert callable(resolve_criterion(torch.nn.CrossEntropyLoss(reduction="sum")))
    assert callable(resolve_criterion(torch.nn.CrossEntropyLoss(weight=torch.ones(3), reduction="sum", ignore_index=255)))
    with pytest.raises(ValueError, match="scalar"):
        resolve_criterion(torch.nn.CrossEntropyLoss(reduction="none"))
    with pytest.raises(ValueError, match=r"label.*weaklysuperviseddl_amd\.nn\.CrossEntropyLoss"):
        resolve_criterion(torch.nn.CrossEntropyLoss(label_smoothing=0.1))
    import weaklysuperviseddl_amd.nn as wnn
    crit = wnn.CrossEntropyLoss(label_smoothing=0.1)
    assert resolve_criterion(crit) is crit


def test_cross_entropy_keywords_and_argument_errors_need_no_device():
    from weaklysuperviseddl_amd import ops
    import weaklysuperviseddl_amd.nn as wnn
    params = inspect.signature(ops.cross_entropy).parameters
    assert list(params)[:3] == ["logits", "labels", "ignore_index"] and params["ignore_index"].default == -100
    for name, default in (("weight", None), ("label_smoothing", 0.0), ("reduction", "mean"), ("pixel_weight", None)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    z, y = torch.zeros(1, 2, 3, 3), torch.zeros(1, 3, 3, dtype=torch.long)
    for kw in ({"reduction": "avg"}, {"reduction": None}, {"label_smoothing": -0.1}, {"label_smoothing": 1.5},
               {"label_smoothing": float("nan")}, {"label_smoothing": "0.1"}):
        with pytest.raises(ValueError):
            ops.cross_entropy(z, y, **kw)
        with pytest.raises(ValueError):
            wnn.CrossEntropyLoss(**kw)
    # shapes and dtypes of the weights are refused before anything is launched (no library call on a host tensor either)
    for kw in ({"weight": torch.ones(3)}, {"weight": torch.ones(2, dtype=torch.float64)}, {"pixel_weight": torch.ones(1, 3, 4)},
               {"pixel_weight": torch.ones(1, 3, 3, dtype=torch.float64)}, {"weight": [1.0, 1.0]}):
        with pytest.raises(ops.WsdlError, match="weight"):
            ops.cross_entropy(z, y, **kw)
    assert inspect.signature(ops.class_weights_from_labels).parameters["mode"].default == "inverse"
    with pytest.raises(ValueError, match="mode"):
        ops.class_weights_from_labels(y, 2, mode="sqrt")
    from weaklysuperviseddl_amd.FullySupervisedModel import SupervisedModel as sm
    p = inspect.signature(sm.run_supervised_training).parameters["criterion"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_loss_objects_that_differ_have_different_plan_keys():
    from weaklysuperviseddl_amd import plan
    import weaklysuperviseddl_amd.nn as wnn
    base = plan.host_scalars(wnn.CrossEntropyLoss())
    assert base == plan.host_scalars(wnn.CrossEntropyLoss())
    assert plan.host_scalars(wnn.CrossEntropyLoss(label_smoothing=0.1)) != base
    assert plan.host_scalars(wnn.CrossEntropyLoss(reduction="sum")) != base
    assert plan.host_scalars(wnn.CrossEntropyLoss(ignore_index=255)) != base
    assert plan.host_scalars(wnn.CrossEntropyLoss(weight=torch.ones(2))) != base
    crit = wnn.CrossEntropyLoss()
    assert crit.pixel_weight is None
    crit.set_pixel_weight(torch.rand(2, 4, 4))
    k1, buf = plan.host_scalars(crit), crit.pixel_weight
    assert k1 != base
    crit.set_pixel_weight(torch.rand(2, 4, 4))                 # same shape: same buffer, new values, same key
    assert crit.pixel_weight is buf and plan.host_scalars(crit) == k1
    crit.set_pixel_weight(torch.rand(2, 4, 5))                 # another shape: another buffer, another key
    assert crit.pixel_weight is not buf and plan.host_scalars(crit) != k1
    crit.set_pixel_weight(None)
    assert plan.host_scalars(crit) == base
