"""The oracle of the view-consistency kernels (tests/consistency_oracle.py) against independent formulations, and the host side
of the feature - no device needed.

  * the warp against ``F.grid_sample(align_corners=False)`` where the two rules coincide (interior pixels: all four taps
    unclamped), and against a per-pixel loop written from the contract;
  * the adjoint by ``<warp(x), g> == <x, adjoint(g)>`` in float64;
  * the three loss kinds against ``F.kl_div`` / ``F.mse_loss`` / ``F.cross_entropy`` under float64 autograd and against
    central differences;
  * ``augment.relative_rows`` against explicit 3 x 3 matrix inverses;
  * every host refusal of ``ops.check_consistency_options``, the two warps and ``wnn.ConsistencyLoss``;
  * the near-tie cap the device test relies on, asserted of the float32 oracle itself.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_oracle as O  # noqa: E402

F = np.float32


def _rows_for(hw, thw):
    return [(n, O.named_row(n, hw, thw)) for n in O.ROW_NAMES]


# ----------------------------------------------------------------------------------------------------------------- the warp
@pytest.mark.parametrize("hw,thw", [((9, 11), (9, 11)), ((12, 10), (17, 23)), ((16, 16), (7, 9))])
def test_warp_oracle_matches_grid_sample_in_the_interior(hw, thw):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3,) + thw).astype(F)
    checked = 0
    for name in ("identity", "flip", "rot+30_x0.5", "rot-30_x2", "half_pixel"):
        row = O.named_row(name, hw, thw)
        val, inside = O.warp_one(x, row, hw)
        t = O.taps(row, thw, hw)
        with np.errstate(all="ignore"):
            xs, ys, _ = O.source_coords(row, thw, hw, "ignore")
        interior = inside & (xs >= 0.5) & (xs < thw[1] - 0.5) & (ys >= 0.5) & (ys < thw[0] - 0.5)
        grid = torch.from_numpy(np.stack([2.0 * xs.astype(np.float64) / thw[1] - 1.0, 2.0 * ys.astype(np.float64) / thw[0] - 1.0], -1))[None]
        ref = TF.grid_sample(torch.from_numpy(x).double()[None], grid, mode="bilinear", padding_mode="border",
                             align_corners=False)[0].numpy()
        assert np.allclose(val[:, interior], ref[:, interior], rtol=0, atol=1e-9 * max(thw)), name
        assert (t["x1"][interior] == t["x0"][interior] + 1).all() and (t["y1"][interior] == t["y0"][interior] + 1).all()
        checked += int(interior.sum())
    assert checked > 0


@pytest.mark.parametrize("fill", ["ignore", "reflect"])
def test_warp_oracle_matches_a_per_pixel_loop(fill):
    hw, thw = (6, 7), (5, 9)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2,) + thw).astype(F)
    labels = rng.integers(0, 5, thw).astype(np.int64)
    h, w = thw
    for name, row in _rows_for(hw, thw):
        got32, inside = O.warp_one(x, row, hw, fill, pad_value=-7.0, photometric=True, dtype=F)
        got_l = O.warp_labels(labels[None], row[None], hw, fill, pad_label=-5)[0]
        r = [F(v) for v in row]
        for oy in range(hw[0]):
            for ox in range(hw[1]):
                with np.errstate(all="ignore"):
                    u, v = F(ox) + F(0.5), F(oy) + F(0.5)
                    xs = F(F(F(r[0] * u) + F(r[1] * v)) + r[2])
                    ys = F(F(F(r[3] * u) + F(r[4] * v)) + r[5])
                    if fill == "reflect":
                        def refl(s, n):
                            P = F(2) * F(n)
                            q = F(np.floor(F(s / P)))
                            rr = F(s - F(P * q))
                            if rr < 0:
                                rr = F(rr + P)
                            if rr >= F(n):
                                rr = F(P - rr)
                            return rr
                        xs, ys = refl(xs, w), refl(ys, h)
                        ins = True
                    else:
                        ins = bool(xs >= 0 and xs < F(w) and ys >= 0 and ys < F(h))
                    ins = ins and bool(np.isfinite(xs)) and bool(np.isfinite(ys))
                assert ins == bool(inside[oy, ox]), (name, oy, ox)
                if not ins:
                    assert (got32[:, oy, ox] == F(-7.0)).all() and got_l[oy, ox] == -5
                    continue
                assert got_l[oy, ox] == labels[min(int(math.floor(ys)), h - 1), min(int(math.floor(xs)), w - 1)]
                xc, yc = F(xs - F(0.5)), F(ys - F(0.5))
                x0, y0 = math.floor(xc), math.floor(yc)
                fx, fy = F(xc - F(x0)), F(yc - F(y0))
                cl = lambda i, n: min(max(i, 0), n - 1)          # noqa: E731
                for c in range(x.shape[0]):
                    v00, v01 = x[c, cl(y0, h), cl(x0, w)], x[c, cl(y0, h), cl(x0 + 1, w)]
                    v10, v11 = x[c, cl(y0 + 1, h), cl(x0, w)], x[c, cl(y0 + 1, h), cl(x0 + 1, w)]
                    top = v00 if fx == 0 else F(v00 + F(fx * F(v01 - v00)))
                    bot = v10 if fx == 0 else F(v10 + F(fx * F(v11 - v10)))
                    val = top if fy == 0 else F(top + F(fy * F(bot - top)))
                    val = F(F(r[6] * val) + r[7])
                    assert got32[c, oy, ox] == val, (name, c, oy, ox)


def test_warp_oracle_identity_keeps_infinities_and_zero_fractions_skip_unused_taps():
    x = np.array([[[1.0, np.inf, -np.inf], [np.nan, 2.0, -0.0]]], dtype=F)
    for dt in (F, np.float64):
        val, inside = O.warp_one(x, O.named_row("identity", (2, 3), (2, 3)), dtype=dt)
        assert inside.all() and np.array_equal(val.astype(F).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("hw,thw", [((5, 7), (5, 7)), ((9, 4), (6, 11)), ((4, 4), (1, 1))])
def test_adjoint_oracle_is_the_adjoint(hw, thw):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2,) + thw).astype(F)
    g = rng.standard_normal((2,) + hw).astype(F)
    for name, row in _rows_for(hw, thw):
        for photometric in (False, True):
            row = row.copy()
            if name not in ("nan",):
                row[6], row[7] = F(1.25), F(0.0)           # (a bias is no part of the linear map)
            val, inside = O.warp_one(x, row, hw, photometric=photometric)
            adj = O.adjoint_one(g, row, thw, photometric=photometric)
            lhs, rhs = float((val * g).sum()), float((x.astype(np.float64) * adj).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (name, photometric, lhs, rhs)
            if not inside.any():
                assert not adj.any()


# ----------------------------------------------------------------------------------------------------------------- the loss
def _torch_loss(z, t, w, kind, teacher_is, T, lam, normalize):
    """The contract in float64 torch operations; z requires grad."""
    B, C, H, W = z.shape
    q = torch.softmax(t / T, 1) if teacher_is == "logits" else t / t.sum(1, keepdim=True)
    if kind == "kl":
        per = TF.kl_div(torch.log_softmax(z, 1), q, reduction="none").sum(1)
    elif kind == "mse":
        per = TF.mse_loss(torch.softmax(z, 1), q, reduction="none").mean(1)
    else:
        per = TF.cross_entropy(z, q.argmax(1), reduction="none")
    N = B * H * W if normalize == "all" else w.sum()
    return lam / N * (w * per).sum()


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("teacher_is", ["logits", "probs"])
@pytest.mark.parametrize("normalize", ["all", "counted"])
def test_loss_oracle_matches_torch_autograd(kind, teacher_is, normalize):
    B, C, H, W = 2, 5, 4, 6
    z, t = O.loss_inputs(B, C, H, W, (H, W), 11, teacher_is)
    T = 0.5 if teacher_is == "logits" else 1.0
    rng = np.random.default_rng(5)
    pw = rng.random((B, H, W)).astype(F)
    inside = rng.random((B, H, W)) > 0.2
    want = O.consistency(z, t, inside, kind=kind, teacher_is=teacher_is, temperature=T, tau=0.9, lam=0.75, normalize=normalize,
                         pixel_weight=pw)
    assert 0 < want["n_counted"] < want["n_inside"] < B * H * W
    zt = torch.from_numpy(z).double().requires_grad_(True)
    loss = _torch_loss(zt, torch.from_numpy(t).double(), torch.from_numpy(want["weight"]), kind, teacher_is, T, 0.75, normalize)
    loss.backward()
    assert abs(loss.item() - float(want["loss"])) <= 1e-13 * max(1.0, abs(loss.item()))
    assert np.abs(zt.grad.numpy() - want["grad"]).max() <= 1e-14
    # the decision itself, from its definition
    q = torch.softmax(torch.from_numpy(t).double() / T, 1) if teacher_is == "logits" else torch.from_numpy(t).double()
    q = q / q.sum(1, keepdim=True)
    assert np.array_equal(want["counted"], inside & (q.max(1).values.numpy() >= np.float64(F(0.9))))
    assert np.array_equal(want["raw_target"], q.argmax(1).numpy())


@pytest.mark.parametrize("kind", O.KINDS)
def test_loss_oracle_gradient_matches_central_differences(kind):
    B, C, H, W = 1, 3, 2, 3
    z, t = O.loss_inputs(B, C, H, W, (H, W), 12)
    kw = dict(kind=kind, temperature=0.5, tau=0.0, lam=1.5, normalize="counted")
    want = O.consistency(z, t, **kw)
    z64, eps = z.astype(np.float64), 1e-6
    for idx in np.ndindex(z.shape):
        zp, zm = z64.copy(), z64.copy()
        zp[idx] += eps
        zm[idx] -= eps
        d = (O.pixel_terms(zp, t, kind, "logits", 0.5)["loss"].sum() - O.pixel_terms(zm, t, kind, "logits", 0.5)["loss"].sum()) / (2 * eps)
        assert abs(d * 1.5 / (B * H * W) - want["grad"][idx]) <= 1e-8, (kind, idx)


def test_loss_oracle_edges():
    z, t = O.loss_inputs(1, 3, 2, 2, (2, 2), 13)
    none = O.consistency(z, t, np.zeros((1, 2, 2), bool), normalize="counted")
    assert none["loss"] == 0 and not none["grad"].any() and none["n_counted"] == 0 and (none["target"] == -100).all()
    z2 = z.copy()
    z2[0, 1, 0, 0] = np.inf
    t2 = t.copy()
    t2[0, 0, 1, 1] = np.nan
    r = O.consistency(z2, t2)
    assert r["n_counted"] == 2 and np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all()
    assert not r["grad"][0, :, 0, 0].any() and not r["grad"][0, :, 1, 1].any()
    big = np.array([40.0, 0.0, -40.0], dtype=F).reshape(1, 3, 1, 1)
    for kind in O.KINDS:
        r = O.consistency(big, -big, kind=kind)
        assert np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all(), kind


def test_float32_oracle_decisions_stay_inside_the_near_tie_cap():
    """What tests/test_hip_consistency.py asks of the device is asked of the float32 oracle first: its counted / target planes
    equal the float64 ones wherever |conf - tau| and the top-two gap exceed twice the standing bound, and at most 0.1 % of a
    case's pixels are exempt (teacher logits 3 * randn: a near-tie has probability about 1e-6 per pixel)."""
    for (B, C, H, W) in O.GEOMS:
        for tau in (0.0, 0.7):
            z, t = O.loss_inputs(B, C, H, W, (H, W), 100 + C)
            rows = np.stack([O.named_row("rot+30_x0.5" if b % 2 else "half_pixel", (H, W), (H, W)) for b in range(B)])
            t32, valid = O.warp_scores(t, rows, dtype=F)
            t64, _ = O.warp_scores(t, rows)
            r32 = O.consistency(z, t32, valid, tau=tau, kind="hard", dtype=F)
            r64 = O.consistency(z, t64, valid, tau=tau, kind="hard")
            ins = valid.astype(bool)
            near = O.near_tie(np.where(ins[:, None], t32, 0), np.where(ins[:, None], t64, 0), r32["conf"].astype(np.float64),
                              r64["conf"], tau) & ins
            assert near.sum() <= 1e-3 * near.size, (B, C, H, W, tau, int(near.sum()))
            assert np.array_equal(r32["counted"][~near], r64["counted"][~near])
            assert np.array_equal(r32["target"][~near], r64["target"][~near])


# ------------------------------------------------------------------------------------------------------------ relative rows
def test_relative_rows_against_explicit_inverses():
    from weaklysuperviseddl_amd.augment import Augment, relative_rows
    g = torch.Generator().manual_seed(7)
    aug = Augment(scale=(0.5, 2.0), rotate=30.0, hflip=0.5, brightness=0.2, contrast=0.2)
    S, T = aug.draw(6, (40, 56), (32, 48), g), aug.draw(6, (40, 56), (24, 24), g)
    got = relative_rows(S, T)
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, 8)

    def mat(r):
        return np.array([[r[0], r[1], r[2]], [r[3], r[4], r[5]], [0, 0, 1]], dtype=np.float64)
    for s, t, r in zip(S.numpy(), T.numpy(), got.numpy()):
        want = np.linalg.inv(mat(t)) @ mat(s)
        assert np.allclose(mat(r)[:2], want[:2], rtol=2.0 ** -22, atol=2.0 ** -22 * 64) and r[6] == 1 and r[7] == 0
    alone = relative_rows(S)
    assert torch.equal(alone[:, :6], S[:, :6]) and (alone[:, 6] == 1).all() and (alone[:, 7] == 0).all()
    # T^-1 o T in float64: every entry within a few 2^-53 x (|entries| up to 56 / |det| down to 1/8) of the identity's - far below
    # float32's spacing at 1, so the ones are exact after the cast and the zeros stay below 1e-12
    same = relative_rows(S, S)[:, :6].numpy()
    assert np.array_equal(same[:, [0, 4]], np.ones((6, 2), dtype=F)) and np.abs(same[:, [1, 2, 3, 5]]).max() <= 1e-12
    with pytest.raises(ValueError, match="student_rows"):
        relative_rows(torch.zeros(3, 6))
    with pytest.raises(ValueError, match="teacher_rows"):
        relative_rows(S, T[:3])
    sing = relative_rows(S[:1], torch.tensor([[0.0, 0, 1, 0, 0, 1, 1, 0]]))
    assert not torch.isfinite(sing[:, :6]).all()


# ---------------------------------------------------------------------------------------------------------- host refusals
def _ok_args():
    z, t = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5)
    return z, t


@pytest.mark.parametrize("change,match", [
    (dict(kind="l2"), "kind"), (dict(teacher_is="probabilities"), "teacher_is"), (dict(normalize="mean"), "normalize"),
    (dict(fill="zeros"), "fill"), (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(tau=-0.1), "tau"), (dict(tau=1.5), "tau"), (dict(tau="x"), "tau"),
    (dict(lam=float("inf")), "lam"), (dict(tau=torch.zeros(2)), "tau as a tensor"), (dict(lam=torch.zeros(1, dtype=torch.float64)), "lam as a tensor"),
    (dict(pixel_weight=torch.zeros(2, 4, 4)), "pixel_weight"), (dict(pixel_weight=torch.zeros(2, 4, 5, dtype=torch.float64)), "pixel_weight"),
    (dict(counts=torch.zeros(3, dtype=torch.int64)), "counts"), (dict(counts=torch.zeros(2, dtype=torch.int32)), "counts"),
    (dict(weight_out=torch.zeros(2, 4, 5, dtype=torch.float64)), "weight_out"), (dict(target_out=torch.zeros(2, 4, 5)), "target_out"),
    (dict(weight_out=torch.zeros(2, 4, 5, requires_grad=True)), "weight_out"),
])
def test_check_consistency_options_refuses_options(change, match):
    from weaklysuperviseddl_amd import ops
    z, t = _ok_args()
    with pytest.raises(ops.WsdlError, match=match):
        ops.check_consistency_options(z, t, **change)


def test_check_consistency_options_refuses_tensors():
    from weaklysuperviseddl_amd import ops
    z, t = _ok_args()
    E = ops.WsdlError
    with pytest.raises(E, match=r"student_logits must be a \(B,C,H,W\)"):
        ops.check_consistency_options(z[0], t)
    with pytest.raises(E, match="teacher must be a"):
        ops.check_consistency_options(z, "t")
    with pytest.raises(E, match="float32"):
        ops.check_consistency_options(z.half(), t)
    with pytest.raises(E, match="float32"):
        ops.check_consistency_options(z, t.double())
    with pytest.raises(E, match="empty"):
        ops.check_consistency_options(z[:, :, :0], t)
    with pytest.raises(E, match="at most 64"):
        ops.check_consistency_options(torch.zeros(1, 65, 2, 2), torch.zeros(1, 65, 2, 2))
    with pytest.raises(E, match="B = 2 and C = 3"):
        ops.check_consistency_options(z, t[:1])
    with pytest.raises(E, match="B = 2 and C = 3"):
        ops.check_consistency_options(z, t[:, :2])
    with pytest.raises(E, match="rows=None"):
        ops.check_consistency_options(z, torch.zeros(2, 3, 8, 5))
    with pytest.raises(E, match="rows must be"):
        ops.check_consistency_options(z, t, torch.zeros(2, 6))
    with pytest.raises(E, match="rows must be"):
        ops.check_consistency_options(z, t, torch.zeros(2, 8, dtype=torch.float64))
    w = torch.zeros(2, 4, 5)
    with pytest.raises(E, match="weight_out shares memory with pixel_weight"):
        ops.check_consistency_options(z, t, pixel_weight=w, weight_out=w)
    big = torch.zeros(2 * 4 * 5 + 2, dtype=torch.int64)
    with pytest.raises(E, match="target_out shares memory with counts"):
        ops.check_consistency_options(z, t, counts=big[:2], target_out=big[1:41].view(2, 4, 5))
    with pytest.raises(E, match="weight_out shares memory with student_logits"):
        ops.check_consistency_options(z, t, weight_out=z.view(-1)[:40].view(2, 4, 5))
    # everything passes the host checks: the place is refused last (no device here, no CPU fallback)
    with pytest.raises(E, match="needs a device tensor"):
        ops.check_consistency_options(z, t, torch.zeros(2, 8), tau=torch.zeros(1), pixel_weight=w)
    with pytest.raises(E, match="needs a device tensor"):
        ops.consistency_loss(z, t)


def test_warps_refuse_on_the_host():
    from weaklysuperviseddl_amd import ops
    E = ops.WsdlError
    x, rows = torch.zeros(2, 3, 4, 5), torch.zeros(2, 8)
    for bad, match in ((dict(scores=x[0]), "rank 4"), (dict(scores=x.double()), "float32"), (dict(scores=x[:, :, :0]), "empty"),
                       (dict(scores=torch.zeros(1, 65, 2, 2), rows=rows[:1]), "at most 64"), (dict(rows=rows[:1]), "rows must be"),
                       (dict(rows=rows.double()), "rows must be"), (dict(fill="zeros"), "fill"), (dict(out_size=(0, 4)), "out_size"),
                       (dict(out_size=(4, 16385)), "out_size"), (dict(pad_value=float("inf")), "pad_value")):
        kw = dict(scores=x, rows=rows)
        kw.update(bad)
        with pytest.raises(E, match=match):
            ops.warp_scores(kw.pop("scores"), kw.pop("rows"), kw.pop("out_size", None), **kw)
    with pytest.raises(E, match="needs a device tensor"):
        ops.warp_scores(x, rows)
    lab = torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(E, match="int64"):
        ops.warp_labels(lab.int(), rows)
    with pytest.raises(E, match="rank 3"):
        ops.warp_labels(lab[0], rows)
    with pytest.raises(E, match="pad_label"):
        ops.warp_labels(lab, rows, pad_label=1.5)
    with pytest.raises(E, match="needs a device tensor"):
        ops.warp_labels(lab, rows)


def test_consistency_module_host_side():
    from weaklysuperviseddl_amd import nn as wnn, plan
    for bad, match in ((dict(kind="l2"), "kind"), (dict(normalize="x"), "normalize"), (dict(fill="x"), "fill"),
                       (dict(teacher_is="x"), "teacher_is"), (dict(temperature=0), "temperature"), (dict(tau=2), "tau"),
                       (dict(lam=float("nan")), "lam")):
        with pytest.raises(ValueError, match=match):
            wnn.ConsistencyLoss(**bad)
    c = wnn.ConsistencyLoss(kind="hard", tau=0.7, lam=0.25, temperature=0.5)
    assert c.knobs.tolist() == [F(0.7), 0.25, 0.5] and c.counts.dtype == torch.int64 and c.teacher_ptr == 0 and c.teacher_shape == ""
    with pytest.raises(ValueError, match="set_teacher"):
        c(torch.zeros(1, 2, 3, 3))
    k0 = plan.host_scalars(c)
    t = torch.randn(2, 3, 4, 5)
    c.set_teacher(t, torch.zeros(2, 8))
    ptr, rptr, kptr = c.teacher_ptr, c.rows_ptr, c.knobs_ptr
    assert ptr == c.teacher.data_ptr() != 0 and c.teacher_shape == "2x3x4x5" and torch.equal(c.teacher, t) and c.teacher is not t
    k1 = plan.host_scalars(c)
    assert k1 != k0
    c.set_teacher(2 * t, torch.ones(2, 8))                           # new contents, the same buffers: the same plan key
    c.set_lam(0.5).set_tau(0.9).set_temperature(2.0)
    assert (c.teacher_ptr, c.rows_ptr, c.knobs_ptr) == (ptr, rptr, kptr) and plan.host_scalars(c) == k1
    assert torch.equal(c.teacher, 2 * t) and c.knobs.tolist() == [F(0.9), 0.5, 2.0]
    c.set_teacher(torch.randn(2, 3, 6, 5))                           # another shape: new buffer, no rows, another key
    assert c.rows is None and c.rows_ptr == 0 and c.teacher_shape == "2x3x6x5" and plan.host_scalars(c) != k1
    c.kind = "kl"
    assert plan.host_scalars(c) != k1
    for call, match in ((lambda: c.set_tau(-1), "tau"), (lambda: c.set_lam(float("inf")), "lam"),
                        (lambda: c.set_temperature(0.0), "temperature"), (lambda: c.set_teacher(t[0]), "teacher must be"),
                        (lambda: c.set_teacher(t, torch.zeros(3, 8)), "rows must be"),
                        (lambda: c.set_teacher(t.double()), "teacher must be float32"),
                        (lambda: c.set_teacher(t.half(), torch.zeros(2, 8)), "teacher must be float32"),
                        (lambda: c.set_teacher(t, torch.zeros(2, 8, dtype=torch.int64)), "rows must be float32")):
        with pytest.raises(ValueError, match=match):
            call()


def test_train_step_consistency_checks_its_arguments():
    from weaklysuperviseddl_amd import nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import train_step_consistency

    class Opt:
        ema = None
    with pytest.raises(ValueError, match="FlatEMA attached"):
        train_step_consistency(None, None, Opt(), None, None, None, consistency=wnn.ConsistencyLoss())

    class Ema:
        model = "m"
    e = Ema()
    o = Opt()
    o.ema = e
    with pytest.raises(ValueError, match="wnn.ConsistencyLoss"):
        train_step_consistency("m", e, o, None, None, None, consistency=lambda a, b: 0)
