"""The view-consistency kernels on the device (csrc/consistency.hip) against the oracle of tests/consistency_oracle.py.

Exact: the ``valid`` planes, ``warp_labels``, the identity warp, the counts, and - away from near-ties - the weight and target
planes.  Everything else is under the project's standing parity bound, per tensor: ``max(4 x |float32 oracle - float64 oracle|,
2^-23 |value|)`` from the float64 oracle, the float32 oracle being the same contract evaluated in float32 (for the warp: the
kernel's own arithmetic, operation for operation).  The worst device-error-to-bound ratios go to the parity report.

Near-ties: whether a pixel is counted hinges on ``conf >= tau`` and its hard target on the order of the two largest teacher
values; the device takes both decisions on the float32-warped teacher values, the float64 oracle on the float64-warped ones.
Where ``|conf - tau|`` or the top-two gap is within twice the bound of that quantity either answer is right; with teacher
logits ``3 * randn`` such pixels have probability about 1e-6 and at most 0.1 % of a case's pixels may be exempt
(tests/test_consistency.py asserts the same cap of the float32 oracle).  Loss and gradient are then compared with the float64
oracle evaluated WITH the device's published weight plane, so a legitimate other decision does not show up as an error.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------------------- warp and adjoint
@pytest.mark.parametrize("geom", O.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_warps_and_adjoint_at_every_geometry_and_row(dev, geom):
    """Every geometry x teacher size (equal, smaller, larger) x named row (identity / resize, flip, +-30 degrees at scale 0.5 and 2, half-pixel shift,
    a view entirely outside, a row of NaN, a singular row - the adjoint's whole-output fallback): valid planes and labels exact,
    values and the adjoint within the standing bound, exact zeros where nothing taps."""
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    B, C, H, W = geom
    rng = np.random.default_rng(sum(geom))
    worst_v = worst_a = 0.0
    for thw in O.teacher_sizes(H, W):
        x = rng.standard_normal((B, C) + thw).astype(F)
        lab = rng.integers(0, 21, (B,) + thw).astype(np.int64)
        dy = rng.standard_normal((B, C, H, W)).astype(F)
        x_dev, lab_dev, dy_dev = _d(x, dev), _d(lab, dev), _d(dy, dev)
        for names, rows in O.row_batches(B, (H, W), thw):
            rows_dev = _d(rows, dev)
            src = x_dev.clone().requires_grad_(True)
            got, valid = ops.warp_scores(src, rows_dev, (H, W), valid=True)
            o32, v32 = O.warp_scores(x, rows, (H, W), dtype=F)
            o64, _ = O.warp_scores(x, rows, (H, W))
            assert np.array_equal(valid.cpu().numpy(), v32), names
            worst_v = max(worst_v, O.ratio(got.detach().cpu().numpy(), o32, o64))
            assert np.array_equal(ops.warp_labels(lab_dev, rows_dev, (H, W)).cpu().numpy(), O.warp_labels(lab, rows, (H, W))), names
            got.backward(dy_dev)
            a64, a32 = O.adjoint(dy, rows, thw), O.adjoint(dy, rows, thw, dtype=F)
            adj = src.grad.cpu().numpy()
            worst_a = max(worst_a, O.ratio(adj, a32, a64))
            assert not adj[a64 == 0].any(), names                          # exact zeros where nothing taps
            assert torch.equal(src.detach(), x_dev)                         # the input is untouched
        # the reflect fill (no padding): one batch per size
        names, rows = O.row_batches(B, (H, W), thw)[0]
        got, valid = ops.warp_scores(x_dev, _d(rows, dev), (H, W), fill="reflect", valid=True, pad_value=-3.0)
        o32, v32 = O.warp_scores(x, rows, (H, W), dtype=F, fill="reflect", pad_value=-3.0)
        o64, _ = O.warp_scores(x, rows, (H, W), fill="reflect", pad_value=-3.0)
        assert np.array_equal(valid.cpu().numpy(), v32)
        worst_v = max(worst_v, O.ratio(got.cpu().numpy(), o32, o64))
        assert np.array_equal(ops.warp_labels(lab_dev, _d(rows, dev), (H, W), fill="reflect").cpu().numpy(),
                              O.warp_labels(lab, rows, (H, W), fill="reflect"))
    report_line(f"warp_scores {geom}: worst device error / bound {worst_v:.3f}; adjoint {worst_a:.3f}")
    assert worst_v <= 1.0 and worst_a <= 1.0, (worst_v, worst_a)


def test_warp_properties(dev):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.augment import IDENTITY_ROW
    B, C, H, W = 3, 4, 13, 70
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, C, H, W)).astype(F)
    x[0, 1, 2, 3], x[1, 0, 0, 0], x[2, 3, 12, 69], x[0, 0, 5, 5] = np.inf, -np.inf, np.inf, -0.0
    x_dev = _d(x, dev)
    ident = torch.tensor([IDENTITY_ROW] * B, device=dev)
    # the identity is bit for bit, infinities and the negative zero included (fx = fy = 0 takes the first tap as it is)
    got, valid = ops.warp_scores(x_dev, ident, valid=True)
    assert _same_bits(got, x_dev) and bool(valid.all())
    # photometric, a pad value, another output size; against the float32 oracle exactly and the float64 one within the bound
    x[~np.isfinite(x)] = 1.5
    x_dev = _d(x, dev)
    rows = np.stack([O.named_row(n, (9, 31), (H, W)) for n in ("rot+30_x0.5", "half_pixel", "rot-30_x2")])
    rows[:, 6], rows[:, 7] = F(1.25), F(-0.5)
    rows_dev = _d(rows, dev)
    got, valid = ops.warp_scores(x_dev, rows_dev, (9, 31), photometric=True, pad_value=7.0, valid=True)
    o32, v32 = O.warp_scores(x, rows, (9, 31), dtype=F, photometric=True, pad_value=7.0)
    o64, _ = O.warp_scores(x, rows, (9, 31), photometric=True, pad_value=7.0)
    assert np.array_equal(valid.cpu().numpy(), v32) and 0 < v32.sum() < v32.size
    assert O.ratio(got.cpu().numpy(), o32, o64) <= 1.0
    assert (got.cpu().numpy()[np.broadcast_to(v32[:, None] == 0, o32.shape)] == 7.0).all()
    plain = ops.warp_scores(x_dev, rows_dev, (9, 31), pad_value=7.0)
    assert not _same_bits(plain, got)
    # out= reuse, two calls bit-identical, independent of B, strided inputs
    buf = torch.empty(B, C, 9, 31, device=dev)
    assert ops.warp_scores(x_dev, rows_dev, (9, 31), photometric=True, pad_value=7.0, out=buf) is buf and _same_bits(buf, got)
    assert _same_bits(ops.warp_scores(x_dev, rows_dev, (9, 31), photometric=True, pad_value=7.0), got)
    one = ops.warp_scores(x_dev[1:2], rows_dev[1:2], (9, 31), photometric=True, pad_value=7.0)
    assert _same_bits(one, got[1:2])
    wide = torch.zeros(B, 2 * C, H, W + 3, device=dev)
    wide[:, ::2, :, :W] = x_dev
    strided = wide[:, ::2, :, :W]
    assert not strided.is_contiguous()
    assert _same_bits(ops.warp_scores(strided, rows_dev, (9, 31), photometric=True, pad_value=7.0), got)
    lab = torch.randint(0, 9, (B, H, W + 3), device=dev)[:, :, :W]
    assert torch.equal(ops.warp_labels(lab, rows_dev, (9, 31)), ops.warp_labels(lab.contiguous(), rows_dev, (9, 31)))
    lbuf = torch.empty(B, 9, 31, dtype=torch.int64, device=dev)
    assert ops.warp_labels(lab, rows_dev, (9, 31), pad_label=255, out=lbuf) is lbuf and int((lbuf == 255).sum()) == int((v32 == 0).sum())
    assert torch.equal(x_dev, _d(x, dev))
    with pytest.raises(ops.WsdlError, match="out shares memory"):
        ops.warp_scores(x_dev, ident, out=x_dev)
    # a backward through the reflect fill is refused; its forward is not
    src = x_dev.clone().requires_grad_(True)
    out = ops.warp_scores(src, rows_dev, (9, 31), fill="reflect")
    with pytest.raises(ops.WsdlError, match="reflect"):
        out.sum().backward()
    with pytest.raises(ops.WsdlError, match="not built"):
        ops.check(ops.lib().wsdl_warp_scores_bwd(out.data_ptr(), rows_dev.data_ptr(), B, C, H, W, 9, 31, 1, 0, src.data_ptr(), None))


# ------------------------------------------------------------------------------------------------------------------ the loss
def _loss_case(dev, geom, thw, rows, *, kind, normalize, teacher_is, T, tau, with_pw, lam=0.75, seed=0):
    """One call on the device and the oracle's answers -> (ratios, exempt fraction)."""
    from weaklysuperviseddl_amd import ops
    B, C, H, W = geom
    z, t = O.loss_inputs(B, C, H, W, thw, seed, teacher_is)
    rng = np.random.default_rng(seed + 1)
    pw = (rng.random((B, H, W)) * (rng.random((B, H, W)) > 0.1)).astype(F) if with_pw else None
    zd = _d(z, dev).requires_grad_(True)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    w_out = torch.empty(B, H, W, device=dev)
    t_out = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    kw = dict(kind=kind, teacher_is=teacher_is, temperature=T, tau=tau, lam=lam, normalize=normalize)
    loss = ops.consistency_loss(zd, _d(t, dev), None if rows is None else _d(rows, dev), pixel_weight=None if pw is None else _d(pw, dev),
                                counts=counts, weight_out=w_out, target_out=t_out, **kw)
    loss.backward()
    if rows is None:
        t32, t64, valid = t, t.astype(np.float64), np.ones((B, H, W), bool)
    else:
        t32, valid = O.warp_scores(t, rows, (H, W), dtype=F)
        t64, _ = O.warp_scores(t, rows, (H, W))
        valid = valid.astype(bool)
    w_dev, tgt_dev = w_out.cpu().numpy(), t_out.cpu().numpy()
    # decisions: the float64 oracle's own, wherever they are not near-ties
    own = O.consistency(z, t64, valid, pixel_weight=pw, **kw)
    own32 = O.consistency(z, t32, valid, pixel_weight=pw, dtype=F, **kw)
    near = O.near_tie(np.where(valid[:, None], t32, 0), np.where(valid[:, None], t64, 0), own32["conf"].astype(np.float64),
                      own["conf"], tau) & valid
    assert near.sum() <= 1e-3 * near.size, (geom, kind, int(near.sum()))
    assert np.array_equal(w_dev[~near], own["weight"].astype(F)[~near])
    assert np.array_equal(tgt_dev[~near], own["target"][~near])
    n_in, n_cnt = (int(v) for v in counts.cpu())
    assert n_in == int(valid.sum()) and n_cnt == int((tgt_dev != -100).sum())
    if not near.any():
        assert n_cnt == own["n_counted"]
    # values: with the device's published weight plane
    r64 = O.consistency(z, t64, valid, weight=w_dev, **kw)
    r32 = O.consistency(z, t32, valid, weight=w_dev, dtype=F, **kw)
    rl = O.ratio(np.array([loss.item()]), np.array([r32["loss"]]), np.array([r64["loss"]]))
    rg = O.ratio(zd.grad.cpu().numpy(), r32["grad"], r64["grad"])
    if n_cnt == 0 or not (w_dev != 0).any():
        assert loss.item() == 0.0 and not zd.grad.any()
    return rl, rg, n_cnt


@pytest.mark.parametrize("kind", O.KINDS)
def test_loss_kinds_against_the_float64_oracle(dev, kind):
    """Each kind x both normalisations x the teacher as logits (T in {0.5, 1}) and as probabilities x with and without pixel
    weights x tau in {0, 0.7}, dealt over the geometries, the three teacher sizes and the row batches (and the direct read)."""
    from conftest import report_line
    combos = [(n, ti, T, pw) for n in ("all", "counted") for ti, T in (("logits", 0.5), ("logits", 1.0), ("probs", 1.0))
              for pw in (False, True)]
    worst_l = worst_g = 0.0
    counted = 0
    for i, geom in enumerate(O.GEOMS):
        B, C, H, W = geom
        for j in range(3):
            k = 3 * i + j + O.KINDS.index(kind)
            normalize, teacher_is, T, with_pw = combos[k % len(combos)]
            thw = O.teacher_sizes(H, W)[(i + j) % 3]
            batches = O.row_batches(B, (H, W), thw)
            rows = None if (j == 2 and thw == (H, W)) else batches[k % len(batches)][1]
            rl, rg, n = _loss_case(dev, geom, thw, rows, kind=kind, normalize=normalize, teacher_is=teacher_is, T=T,
                                   tau=(0.0, 0.7)[k % 2], with_pw=with_pw, seed=1000 + k)
            worst_l, worst_g, counted = max(worst_l, rl), max(worst_g, rg), counted + n
    # every combination once more at one mid-sized geometry, so that none depends on the deal above
    geom = (3, 3, 37, 53)
    for k, (normalize, teacher_is, T, with_pw) in enumerate(combos):
        thw = O.teacher_sizes(37, 53)[k % 3]
        rows = O.row_batches(3, (37, 53), thw)[k % 3][1]
        rl, rg, n = _loss_case(dev, geom, thw, rows, kind=kind, normalize=normalize, teacher_is=teacher_is, T=T,
                               tau=(0.7, 0.0)[k % 2], with_pw=with_pw, seed=2000 + k)
        worst_l, worst_g, counted = max(worst_l, rl), max(worst_g, rg), counted + n
    report_line(f"consistency_loss {kind}: worst device error / bound, loss {worst_l:.3f}, gradient {worst_g:.3f} ({counted} counted pixels)")
    assert counted > 0 and worst_l <= 1.0 and worst_g <= 1.0, (worst_l, worst_g)


def test_fused_warp_equals_the_unfused_composition_bit_for_bit(dev):
    from weaklysuperviseddl_amd import ops
    for geom, seed in (((3, 3, 37, 53), 1), ((2, 21, 64, 64), 2), ((2, 2, 96, 130), 3), ((1, 64, 9, 11), 4)):
        B, C, H, W = geom
        for thw in O.teacher_sizes(H, W):
            z, t = O.loss_inputs(B, C, H, W, thw, seed)
            for kind, (names, rows) in zip(O.KINDS + ("kl",), O.row_batches(B, (H, W), thw)):
                rows_dev, t_dev = _d(rows, dev), _d(t, dev)
                outs = []
                for fused in (True, False):
                    zd = _d(z, dev).requires_grad_(True)
                    counts = torch.zeros(2, dtype=torch.int64, device=dev)
                    if fused:
                        loss = ops.consistency_loss(zd, t_dev, rows_dev, kind=kind, tau=0.7, normalize="counted", counts=counts)
                    else:                       # NaN padding: a pixel outside is uncounted as a non-finite teacher value
                        warped = ops.warp_scores(t_dev, rows_dev, (H, W), pad_value=float("nan"))
                        loss = ops.consistency_loss(zd, warped, kind=kind, tau=0.7, normalize="counted", counts=counts)
                    loss.backward()
                    outs.append((loss.detach(), zd.grad, int(counts[1])))
                assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2], (geom, names)


def test_loss_edges(dev):
    from weaklysuperviseddl_amd import ops
    B, C, H, W = 2, 3, 5, 7
    z, t = O.loss_inputs(B, C, H, W, (H, W), 7)
    t_dev = _d(t, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(zz, tt=t_dev, rows=None, **kw):
        zd = zz.clone().requires_grad_(True)
        loss = ops.consistency_loss(zd, tt, rows, counts=counts, **kw)
        loss.backward()
        return loss.detach(), zd.grad, counts.tolist()
    z_dev = _d(z, dev)
    # no counted pixel: a view entirely outside, a row of NaN, a confidence nobody reaches - 0 and exact zero gradients
    for name in ("outside", "nan"):
        rows = _d(np.stack([O.named_row(name, (H, W), (H, W))] * B), dev)
        for normalize in ("all", "counted"):
            for kind in O.KINDS:
                loss, grad, c = call(z_dev, rows=rows, normalize=normalize, kind=kind)
                assert float(loss) == 0.0 and not grad.any() and c == [0, 0], (name, normalize, kind)
    flat = torch.zeros_like(t_dev)
    loss, grad, c = call(z_dev, tt=flat, tau=0.5, normalize="counted")            # conf = 1/3 everywhere
    assert float(loss) == 0.0 and not grad.any() and c == [B * H * W, 0]
    # two calls give the same bits
    a, b = call(z_dev, kind="mse", tau=0.3), call(z_dev, kind="mse", tau=0.3)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2] == b[2]
    # non-finite logits on either side are uncounted and leave everything else finite
    z2, t2 = z_dev.clone(), t_dev.clone()
    z2[0, 1, 0, 0], z2[1, 2, 4, 6], t2[0, 0, 2, 2], t2[1, 1, 3, 3] = float("inf"), float("nan"), float("nan"), float("-inf")
    for kind in O.KINDS:
        loss, grad, c = call(z2, tt=t2, kind=kind, normalize="counted")
        assert c == [B * H * W, B * H * W - 4] and bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), kind
        for (b_, y, x_) in ((0, 0, 0), (1, 4, 6), (0, 2, 2), (1, 3, 3)):
            assert not grad[b_, :, y, x_].any()
    # logit gaps of +-40 stay finite, and agree with the oracle
    big = np.zeros((1, 3, 1, 2), dtype=F)
    big[0, :, 0, 0], big[0, :, 0, 1] = (40, 0, -40), (-40, 40, 0)
    for kind in O.KINDS:
        loss, grad, c = call(_d(big, dev), tt=_d(-big, dev), kind=kind, temperature=0.5)
        want = O.consistency(big, -big.astype(np.float64), kind=kind, temperature=0.5)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and c == [2, 2]
        assert abs(float(loss) - want["loss"]) <= 2.0 ** -23 * abs(want["loss"])
        assert np.abs(grad.cpu().numpy() - want["grad"]).max() <= 2.0 ** -23 * np.abs(want["grad"]).max()
    # knobs as device floats: lam = 0 gives 0 and zero gradients, never NaN; a changed float changes the result, not the call
    lam, tau = torch.zeros(1, device=dev), torch.full((1,), 0.5, device=dev)
    loss, grad, c = call(z_dev, lam=lam, tau=tau)
    assert float(loss) == 0.0 and not grad.any() and 0 < c[1] < c[0]
    lam.fill_(2.0)
    l2, g2, c2 = call(z_dev, lam=lam, tau=tau)
    l1, g1, c1 = call(z_dev, lam=2.0, tau=0.5)
    assert float(l2) > 0 and _same_bits(l2, l1) and _same_bits(g2, g1) and c2 == c1 == c
    # strided student logits, the teacher untouched, no gradient wanted
    wide = torch.zeros(B, 2 * C, H, W, device=dev)
    wide[:, ::2] = z_dev
    assert _same_bits(call(wide[:, ::2], lam=2.0, tau=0.5)[0], l1)
    with torch.no_grad():
        assert _same_bits(ops.consistency_loss(z_dev, t_dev, lam=2.0, tau=0.5), l1)
    assert torch.equal(t_dev, _d(t, dev)) and torch.equal(z_dev, _d(z, dev))


# ------------------------------------------------------------------------------------------------------- module, autograd chain
def test_module_equals_the_op_and_autograd_chains_through_the_warp(dev):
    from conftest import report_line
    from weaklysuperviseddl_amd import nn as wnn, ops
    B, C, H, W = 2, 5, 12, 17
    thw = (9, 20)
    z, t = O.loss_inputs(B, C, H, W, thw, 21)
    rows = np.stack([O.named_row("rot+30_x0.5", (H, W), thw), O.named_row("half_pixel", (H, W), thw)])
    z_dev, t_dev, rows_dev = _d(z, dev), _d(t, dev), _d(rows, dev)
    pw = torch.rand(B, H, W, device=dev)
    crit = wnn.ConsistencyLoss(kind="mse", temperature=0.5, tau=0.6, lam=0.3, normalize="counted").to(dev)
    crit.set_teacher(t_dev, rows_dev).set_pixel_weight(pw)
    za, zb = z_dev.clone().requires_grad_(True), z_dev.clone().requires_grad_(True)
    la = crit(za, None)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    lb = ops.consistency_loss(zb, t_dev, rows_dev, kind="mse", temperature=0.5, tau=0.6, lam=0.3, normalize="counted", pixel_weight=pw,
                              counts=counts)
    la.backward()
    lb.backward()
    assert _same_bits(la, lb) and _same_bits(za.grad, zb.grad) and torch.equal(crit.counts, counts) and int(counts[1]) > 0
    ptr = crit.teacher.data_ptr()
    crit.set_teacher(2 * t_dev, rows_dev).set_lam(0.6)
    assert crit.teacher.data_ptr() == ptr and not _same_bits(crit(z_dev), la)
    # SEAM-style chain: the student's map is itself a warp of a map that needs the gradient - d loss / d x = adjoint(d loss / d z)
    xs = (3.0 * np.random.default_rng(22).standard_normal((B, C) + thw)).astype(F)
    x_dev = _d(xs, dev).requires_grad_(True)
    w_out = torch.empty(B, H, W, device=dev)
    zw = ops.warp_scores(x_dev, rows_dev, (H, W))
    loss = ops.consistency_loss(zw, _d(z, dev), kind="kl", weight_out=w_out)
    loss.backward()
    z32, _ = O.warp_scores(xs, rows, (H, W), dtype=F)
    z64, _ = O.warp_scores(xs, rows, (H, W))
    r64 = O.consistency(z64, z, weight=w_out.cpu().numpy())
    r32 = O.consistency(z32, z, weight=w_out.cpu().numpy(), dtype=F)
    a64, a32 = O.adjoint(r64["grad"], rows, thw), O.adjoint(r32["grad"].astype(F), rows, thw, dtype=F)
    ratio = O.ratio(x_dev.grad.cpu().numpy(), a32, a64)
    report_line(f"warp_scores -> consistency_loss autograd chain: worst device error / bound {ratio:.3f}")
    assert ratio <= 1.0 and bool(x_dev.grad.any())


# --------------------------------------------------------------------------------------------------------- the training steps
def _batch(B, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, S, S, generator=g)
    masks = (torch.rand(B, S, S, generator=g) > 0.5).long() * 255
    return img.to(dev), masks.to(dev)


def _deeplab(dev, with_ema=False):
    from weaklysuperviseddl_amd import ema as E
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    torch.manual_seed(0)
    model = build_segmentation_model().to(dev).train()
    opt = make_optimizer(model, lr=1e-4)
    avg = E.FlatEMA(opt, model, build_segmentation_model().to(dev), decay=0.5, warmup=False) if with_ema else None
    return model, opt, avg


def _planned(opt):
    return next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)


def _view_rows(B, S, dev, seed):
    from weaklysuperviseddl_amd.augment import Augment
    g = torch.Generator().manual_seed(seed)
    return Augment(scale=(0.6, 0.9), rotate=20.0, hflip=0.5, brightness=0.1, contrast=0.1).draw(B, (S, S), (S, S), g).to(dev)


def test_train_step_with_the_consistency_term_replays_one_plan(dev):
    """``train_step(..., extra_loss=wnn.ConsistencyLoss)`` on a 64 x 64 batch: the planned run equals the eager one bit for bit;
    the plan recorded in the third call is replayed after ``set_teacher`` with new contents and after ``set_lam`` / ``set_tau``,
    and another ``kind`` records a new one."""
    from weaklysuperviseddl_amd import nn as wnn, plan
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    B, S = 2, 64
    batches = [_batch(B, S, dev, s) for s in (1, 2, 3)]
    teachers = [3.0 * torch.randn(B, 2, S, S, generator=torch.Generator().manual_seed(10 + s)).to(dev) for s in range(3)]
    rows = _view_rows(B, S, dev, 5)

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            model, opt, _ = _deeplab(dev)
            cons = wnn.ConsistencyLoss(kind="kl", tau=0.6, lam=0.5).to(dev)
            torch.manual_seed(1234)
            losses, marks = [], []
            for i in range(8):
                img, m = batches[i % 3]
                cons.set_teacher(teachers[i % 3], rows)
                if i == 4:
                    cons.set_lam(1.5).set_tau(0.8)
                if i == 6:
                    cons.kind = "hard"
                losses.append(float(train_step(model, opt, img, m, extra_loss=cons)))
                st = _planned(opt)
                marks.append(None if st is None else (st.records, st.replays, st.disabled))
            return opt, cons, losses, marks
        finally:
            plan.PLAN_STEP[0] = old
    o0, c0, l0, _ = run(False)
    o1, c1, l1, marks = run(True)
    assert all(np.isfinite(l1)) and l0 == l1 and torch.equal(o0.flat_param, o1.flat_param)
    assert torch.equal(c0.counts, c1.counts) and 0 < int(c1.counts[1]) < int(c1.counts[0]) <= B * S * S
    assert all(m[2] is None for m in marks), marks
    # third call records; 4th, 5th (new knobs), 6th replay; the new kind is eager once, then records
    assert [m[:2] for m in marks] == [(0, 0), (0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 3), (2, 3)], marks
    assert l1[4] != l1[3]


def test_train_step_consistency_and_the_unchanged_defaults(dev):
    """Two calls of ``train_step_consistency`` equal their composition from the public pieces; and ``train_step`` /
    ``train_step_mean_teacher`` without the new arguments give the same bits before and after the feature has been used."""
    from weaklysuperviseddl_amd import nn as wnn, ops
    from weaklysuperviseddl_amd.TraditionalModel import train_step, train_step_consistency, train_step_mean_teacher
    B, S = 2, 64
    batches = [_batch(B, S, dev, s) for s in (1, 2)]
    rows = [_view_rows(B, S, dev, 7), _view_rows(B, S, dev, 8)]

    def defaults():
        model, opt, avg = _deeplab(dev, with_ema=True)
        torch.manual_seed(99)
        out = [float(train_step(model, opt, *batches[0])), float(train_step_mean_teacher(model, avg, opt, *batches[1], tau=0.5))]
        return out, opt.flat_param.clone(), avg.ema_param.clone()
    before = defaults()

    def run(composed):
        model, opt, avg = _deeplab(dev, with_ema=True)
        cons = wnn.ConsistencyLoss(kind="kl", tau=0.5, lam=1.0).to(dev)          # (two classes: every finite pixel is confident)
        torch.manual_seed(1234)
        losses = []
        for (img, m), r in zip(batches, rows):
            if composed:
                with torch.no_grad():
                    logits = avg.teacher(img)["out"]
                view = ops.warp_scores(img, r, photometric=True)
                labels = ops.warp_labels(m.long(), r)
                cons.set_teacher(logits, r)
                losses.append(float(train_step(model, opt, view, labels, extra_loss=cons)))
            else:
                losses.append(float(train_step_consistency(model, avg, opt, img, m, r, consistency=cons)))
        return losses, opt.flat_param.clone(), avg.ema_param.clone(), cons.counts.clone()
    a, b = run(True), run(False)
    assert all(np.isfinite(a[0])) and a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert 0 < int(b[3][1]) == int(b[3][0]) < B * S * S                   # the view does leave the image somewhere
    after = defaults()
    assert before[0] == after[0] and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
