"""Pixel mining without a device: the numpy oracle (tests/pixel_mining_oracle.py) against a torch float64 formulation
(log_softmax, sort, masked weighted mean, autograd), the exact k-th value against a sort, option validation, the plan key of
``wnn.MinedCrossEntropyLoss`` and the trainer's ``criterion=`` keyword."""
import inspect
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_mining_oracle import kth_value_exact, mined_ce, rank  # noqa: E402


def make_case(shape, seed, ignore_index=-100, scale=3.0):
    """As make_case of tests/test_hip_weighted_ce.py."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g) * scale
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.2] = ignore_index
    w = torch.rand(C, generator=g) + 0.25
    p = torch.rand(B, H, W, generator=g) + 0.05
    return z, y, w, p


def torch_mined(z, y, mode, thresh, min_kept, drop_frac, scope, weight, eps, pw, reduction):
    """The formulation a torch user writes: reduction='none', sort, a mask, a weighted mean; float64, autograd."""
    B, C, H, W = z.shape
    zt = z.double().requires_grad_(True)
    logs = torch.log_softmax(zt, 1)
    p = torch.ones(B, H, W, dtype=torch.float64) if pw is None else pw.double()
    v = (y != -100) & (p != 0)
    ys = torch.where(v, y, torch.zeros_like(y))
    nll = -logs.gather(1, ys[:, None]).squeeze(1)
    S = B if scope == "image" else 1
    nl, vv = nll.detach().reshape(S, -1), v.reshape(S, -1)
    kept = torch.zeros_like(vv)
    for s in range(S):
        c, _ = torch.sort(nl[s][vv[s]], descending=True)
        n = c.numel()
        if mode == "hard":
            K = min(n, min_kept * (B if scope == "batch" else 1))
            tau = c[K - 1].item() if K else float("inf")
            if thresh is not None:
                tau = min(tau, -float(np.log(np.float64(thresh))))
            kept[s] = vv[s] & (nl[s] >= tau)
        else:
            K = min(n, 1 + int(np.floor(np.float64(drop_frac) * n)))
            kept[s] = vv[s] & (nl[s] <= c[K - 1]) if K else torch.zeros_like(vv[s])
    m = kept.reshape(B, H, W).double() * p
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    pix = F.cross_entropy(zt, ys, weight=w, reduction="none", label_smoothing=eps) * m
    loss = pix.sum() / (m * w[ys]).sum() if reduction == "mean" else pix.sum()
    loss.backward()
    return loss.detach().numpy(), zt.grad.numpy(), kept.sum(1).numpy()


VARIANTS = [("hard", 0.7, 0, 0.0), ("hard", 0.7, 9, 0.0), ("hard", None, 5, 0.0), ("hard", None, 10 ** 6, 0.0), ("hard", 0.3, 0, 0.0),
            ("trim", None, 0, 0.0), ("trim", None, 0, 0.1), ("trim", None, 0, 0.5)]


@pytest.mark.parametrize("C", (2, 3, 9))
def test_oracle_equals_the_torch_formulation(C):
    z, y, w, p = make_case((3, C, 9, 13), 70 + C)
    p[0, :2] = 0.0                                           # weight 0: no candidate
    for (mode, thresh, min_kept, drop), scope, full, reduction in itertools.product(VARIANTS, ("batch", "image"), (False, True),
                                                                                     ("mean", "sum")):
        weight, eps, pw = (w, 0.1, p) if full else (None, 0.0, None)
        res = mined_ce(z.numpy(), y.numpy(), -100, mode, thresh, min_kept, drop, scope, None if weight is None else weight.numpy(),
                       eps, None if pw is None else pw.numpy(), reduction)
        loss, grad, kept = torch_mined(z, y, mode, thresh, min_kept, drop, scope, weight, eps, pw, reduction)
        what = (mode, thresh, min_kept, drop, scope, full, reduction)
        assert np.array_equal(res["kept"], kept), what
        np.testing.assert_allclose(res["loss"], loss, rtol=1e-12, err_msg=str(what))
        np.testing.assert_allclose(res["grad"], grad, rtol=1e-10, atol=1e-15, err_msg=str(what))
        if mode == "trim":
            assert (res["n_valid"] - res["kept"] <= np.floor(drop * res["n_valid"])).all(), what
        elif min_kept:
            assert (res["kept"] >= np.minimum(res["n_valid"], min_kept * (3 if scope == "batch" else 1))).all(), what


def test_oracle_edges():
    z, y, w, p = make_case((2, 3, 5, 7), 3)
    # drop_frac = 0, and hard without thresh and min_kept >= n: the plain cross entropy
    plain = F.cross_entropy(z.double(), y).item()
    assert abs(mined_ce(z.numpy(), y.numpy(), mode="trim")["loss"] - plain) < 1e-14
    assert abs(mined_ce(z.numpy(), y.numpy(), mode="hard", min_kept=35)["loss"] - plain) < 1e-14
    # nothing valid: 0/0 for mean, 0 for sum, threshold +inf, nothing kept
    yi = np.full((2, 5, 7), -100)
    for mode, scope in itertools.product(("hard", "trim"), ("batch", "image")):
        r = mined_ce(z.numpy(), yi, mode=mode, min_kept=4, drop_frac=0.25 if mode == "trim" else 0.0, scope=scope)
        assert np.isnan(r["loss"]) and not r["kept"].any() and np.isposinf(r["threshold"]).all() and not r["grad"].any()
        assert mined_ce(z.numpy(), yi, mode=mode, scope=scope, reduction="sum")["loss"] == 0.0
    # ties are kept: every pixel the same logits and label
    zt = np.tile(z.numpy()[:1, :, :1, :1], (2, 1, 5, 7))
    r = mined_ce(zt, np.ones((2, 5, 7), dtype=np.int64), mode="hard", min_kept=3)
    assert r["kept"][0] == 70
    r = mined_ce(zt, np.ones((2, 5, 7), dtype=np.int64), mode="trim", drop_frac=0.5)
    assert r["kept"][0] == 70


def test_kth_value_exact_against_a_sort():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1001).astype(np.float32)
    x[::7] = np.nan
    x[5] = np.inf
    valid = rng.random(1001) < 0.8
    c = np.sort(x[valid & ~np.isnan(x)])
    n = c.size
    for k, frac, largest in itertools.product((0, 1, 17, n, n + 5), (0.0, 0.25, 0.5, 1.0), (True, False)):
        v, nn = kth_value_exact(x, k, frac, largest, valid)
        K = min(n, k + int(np.floor(frac * n)))
        assert nn == n and K == rank(n, k, frac)
        if K == 0:
            assert v == (np.inf if largest else -np.inf)
        else:
            assert v == (c[n - K] if largest else c[K - 1]) and v.dtype == np.float32
    assert kth_value_exact(np.full(4, np.nan, np.float32), 1)[1] == 0


def test_option_validation_raises_on_the_host():
    from weaklysuperviseddl_amd import ops
    import weaklysuperviseddl_amd.nn as wnn
    z, y = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    bad = (dict(mode="soft"), dict(mode="hard", thresh=0.0), dict(mode="hard", thresh=1.5), dict(mode="hard", thresh="0.7"),
           dict(mode="hard", min_kept=-1), dict(mode="hard", min_kept=1.5), dict(mode="trim", drop_frac=1.0),
           dict(mode="trim", drop_frac=-0.1), dict(mode="trim", scope="pixel"), dict(mode="trim", reduction="none"),
           dict(mode="trim", reduction="avg"), dict(mode="trim", label_smoothing=2.0))
    for kw in bad:
        with pytest.raises(ValueError):
            ops.cross_entropy_mined(z, y, **kw)
        with pytest.raises(ValueError):
            wnn.MinedCrossEntropyLoss(**kw)
    with pytest.raises(TypeError):
        ops.cross_entropy_mined(z, y)                                       # mode is required
    for kw in (dict(k=-1), dict(k=1.0), dict(frac=1.5), dict(frac=-0.5), dict(segments=0)):
        with pytest.raises(ValueError):
            ops.kth_value(z, **kw)
    with pytest.raises(ops.WsdlError):                                      # valid options, host tensors: no CPU fallback
        ops.cross_entropy_mined(z, y, mode="hard", thresh=0.7)
    crit = wnn.MinedCrossEntropyLoss(mode="trim", drop_frac=0.2)
    crit.drop_frac = 1.5                                                    # assigned after construction: checked at the call
    with pytest.raises(ValueError):
        crit(z, y)
    with pytest.raises(ValueError):
        wnn.MinedCrossEntropyLoss(weight=torch.ones(2, 2))
    with pytest.raises(ValueError):
        wnn.MinedCrossEntropyLoss().set_pixel_weight(torch.ones(4, 4))


def test_every_option_is_part_of_the_plan_key():
    from weaklysuperviseddl_amd import plan
    import weaklysuperviseddl_amd.nn as wnn
    crit = wnn.MinedCrossEntropyLoss(mode="hard", thresh=0.7, min_kept=100)
    assert (crit.mode, crit.thresh, crit.min_kept, crit.drop_frac, crit.scope, crit.reduction) == ("hard", 0.7, 100, 0.0, "batch", "mean")
    seen = {plan.host_scalars(crit)}
    for name, value in (("drop_frac", 0.25), ("min_kept", 7), ("thresh", 0.5), ("thresh", None), ("scope", "image"), ("mode", "trim"),
                        ("label_smoothing", 0.1), ("reduction", "sum"), ("ignore_index", 255)):
        setattr(crit, name, value)
        key = plan.host_scalars(crit)
        assert key not in seen, name
        seen.add(key)
    # the buffers' addresses too: a replaced pixel-weight buffer is another plan, a refilled one is not
    crit.set_pixel_weight(torch.ones(2, 4, 4))
    key = plan.host_scalars(crit)
    assert key not in seen
    crit.set_pixel_weight(torch.zeros(2, 4, 4))
    assert plan.host_scalars(crit) == key
    crit.set_pixel_weight(torch.ones(3, 4, 4))
    assert plan.host_scalars(crit) != key
    assert not [k for k, _ in crit.state_dict().items() if k != "weight"]      # statistics and maps are not checkpointed


def test_trainer_takes_a_criterion_and_keeps_its_positional_signature():
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import train_segmentation_model, resolve_criterion
    import weaklysuperviseddl_amd.nn as wnn
    params = list(inspect.signature(train_segmentation_model).parameters.values())
    positional = [(p.name, p.default) for p in params if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional == [("loss_fn", inspect.Parameter.empty), ("run_id", inspect.Parameter.empty), ("lr", 1e-4), ("num_epochs", 10),
                          ("batch_size", 4), ("val_split", 0.2)]
    crit_p = {p.name: p for p in params}["criterion"]
    assert crit_p.kind is crit_p.KEYWORD_ONLY and crit_p.default is None
    crit = wnn.MinedCrossEntropyLoss(mode="trim", drop_frac=0.2)
    assert resolve_criterion(crit) is crit
    src = inspect.getsource(train_segmentation_model)
    assert "criterion=criterion" in src
