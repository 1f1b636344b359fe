"""AffinityNet ops without a device: the pair set, the oracle of tests/affinity_oracle.py against plain loops and against PSA's
dense matrix power, and the host-side refusals."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_oracle as ao  # noqa: E402


def test_offsets():
    from weaklysuperviseddl_amd import ops
    assert ops.affinity_offsets(2) == [(0, 1), (1, -1), (1, 0), (1, 1)]
    assert len(ops.affinity_offsets(5)) == 34 and len(ops.affinity_offsets(8)) == 96
    for r in range(2, 9):
        offs = ops.affinity_offsets(r)
        assert offs == ao.offsets(r) and len(set(offs)) == len(offs)
        assert all((-dy, -dx) not in offs for dy, dx in offs)                 # never an offset and its negation
        disc = {(y, x) for y in range(-r, r + 1) for x in range(-r, r + 1) if (y, x) != (0, 0) and x * x + y * y < r * r}
        assert set(offs) | {(-dy, -dx) for dy, dx in offs} == disc            # both orientations: the whole disc
        assert offs[:r - 1] == [(0, x) for x in range(1, r)] and offs == sorted(offs)
    for bad in (1, 9, 5.0, True, None):
        with pytest.raises(ops.WsdlError):
            ops.affinity_offsets(bad)


def loop_affinity(feat, radius):
    B, D, h, w = feat.shape
    offs = ao.offsets(radius)
    out = torch.zeros(B, len(offs), h, w, dtype=torch.float64)
    for b in range(B):
        for j, (dy, dx) in enumerate(offs):
            for y in range(h):
                for x in range(w):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        s = sum(abs(float(feat[b, d, y, x]) - float(feat[b, d, y + dy, x + dx])) for d in range(D))
                        out[b, j, y, x] = math.exp(-s / D)
    return out


def loop_kind(a, b, ignore):
    if a == ignore or b == ignore:
        return None
    if a != b:
        return 2
    return 0 if a == 0 else (1 if a > 0 else None)


def loop_loss_and_counts(aff, labels, radius, ignore=255, weights=(0.25, 0.25, 0.5), eps=1e-5):
    B, P, h, w = aff.shape
    sums, counts = [0.0, 0.0, 0.0], [0, 0, 0]
    for b in range(B):
        for j, (dy, dx) in enumerate(ao.offsets(radius)):
            for y in range(h):
                for x in range(w):
                    if not (0 <= y + dy < h and 0 <= x + dx < w):
                        continue
                    k = loop_kind(int(labels[b, y, x]), int(labels[b, y + dy, x + dx]), ignore)
                    if k is None:
                        continue
                    a = float(aff[b, j, y, x])
                    counts[k] += 1
                    sums[k] += -math.log(1 + eps - a) if k == 2 else -math.log(a + eps)
    return sum(weights[k] * sums[k] / (counts[k] + eps) for k in range(3)), counts


@pytest.mark.parametrize("radius", (2, 3, 5))
def test_oracle_slices_equal_per_pixel_loops(radius):
    feat = ao.make_features(2, 3, 4, 5, 1)
    labels = ao.make_labels(2, 4, 5, 2)
    a = ao.affinity(feat, radius)
    assert (a - loop_affinity(feat, radius)).abs().max().item() < 1e-15
    want_L, want_n = loop_loss_and_counts(a, labels, radius)
    L, g = ao.loss(feat, labels, radius)
    assert abs(L.item() - want_L) < 1e-13 and ao.pair_counts(labels, radius).tolist() == want_n
    assert sum(want_n) > 0 and g.abs().max().item() > 0
    # the closed-form gradient of the header: (1/D) sum over the full disc of c sign(f(p) - f(q))
    n = ao.pair_counts(labels, radius).double()
    s = torch.tensor([0.25, 0.25, 0.5], dtype=torch.float64) / (n + 1e-5)
    kinds = ao.pair_kinds(labels, radius)
    c = kinds[0] * s[0] * a / (a + 1e-5) + kinds[1] * s[1] * a / (a + 1e-5) - kinds[2] * s[2] * a / (1 + 1e-5 - a)
    f = feat.double()
    want = torch.zeros_like(f)
    for j, (dy, dx) in enumerate(ao.offsets(radius)):
        win = ao.window(4, 5, dy, dx)
        if win is None:
            continue
        ys, xs, yt, xt = win
        t = c[:, j:j + 1, ys, xs] * torch.sign(f[:, :, ys, xs] - f[:, :, yt, xt]) / 3
        want[:, :, ys, xs] += t
        want[:, :, yt, xt] -= t
    assert (g - want).abs().max().item() < 1e-14


def test_empty_kinds_give_zero():
    feat = ao.make_features(1, 3, 5, 6, 3)
    L, g = ao.loss(feat, ao.make_labels(1, 5, 6, 0, "ignored"), 3)
    assert L.item() == 0.0 and not g.any()
    labels = ao.make_labels(1, 5, 6, 4, "no_bg")
    n = ao.pair_counts(labels, 3).tolist()
    L, _ = ao.loss(feat, labels, 3)
    want, want_n = loop_loss_and_counts(ao.affinity(feat, 3), labels, 3)
    assert n == want_n and n[0] == 0 and n[1] > 0 and n[2] > 0 and abs(L.item() - want) < 1e-13
    assert ao.pair_counts(torch.zeros(1, 1, 1, dtype=torch.int64), 5).tolist() == [0, 0, 0]


def test_stencil_walk_equals_the_dense_matrix_power():
    feat = ao.make_features(1, 6, 7, 9, 5)
    m = ao.make_scores(1, 3, 7, 9, 6)
    for radius, beta in ((5, 8.0), (2, 1.0), (8, 8.0)):
        a = ao.affinity(feat, radius)
        t = ao.transitions(a, beta, radius)
        assert (t.sum(dim=1) - 1).abs().max().item() < 1e-14 and t.min().item() >= 0
        stencil = ao.walk(t, m, (16,), radius)[16]
        dense = ao.dense_walk(a, m, beta, 16, radius)
        assert (stencil - dense).abs().max().item() < 1e-12
    const = torch.full((1, 2, 7, 9), 0.625, dtype=torch.float64)
    assert (ao.walk(t, const, (16,), 8)[16] - 0.625).abs().max().item() < 1e-14


def test_check_affinity_options_refusals():
    from weaklysuperviseddl_amd import ops
    f, lab, m = torch.zeros(2, 4, 6, 6), torch.zeros(2, 6, 6, dtype=torch.int64), torch.zeros(2, 3, 6, 6)
    assert ops.check_affinity_options(5, feat=f, labels=lab, scores=m, beta=8.0, num_iter=256) == 34
    aff, trans = torch.zeros(2, 4, 6, 6), torch.zeros(2, 9, 6, 6)
    assert ops.check_affinity_options(2, aff=aff, trans=trans, scores=m, out=torch.empty(2, 3, 6, 6)) == 4
    for kw in (dict(radius=1), dict(radius=9), dict(radius=2.0), dict(beta=0.0), dict(beta=float("nan")), dict(num_iter=-1),
               dict(num_iter=1.5), dict(weights=(1, 2)), dict(weights=(1, 2, float("inf"))), dict(eps=0.0),
               dict(scores=torch.zeros(2, 33, 6, 6)), dict(feat=torch.zeros(2, 1025, 6, 6)), dict(feat=f, scores=torch.zeros(2, 3, 6, 7)),
               dict(feat=f, scores=torch.zeros(1, 3, 6, 6)), dict(feat=f, labels=torch.zeros(2, 6, 6)), dict(feat=f.double()),
               dict(feat=f, labels=torch.zeros(2, 1, 6, 6, dtype=torch.int64)), dict(aff=torch.zeros(2, 34, 6, 6), radius=2),
               dict(trans=torch.zeros(2, 68, 6, 6)), dict(feat=torch.zeros(2, 4, 0, 6)), dict(feat=torch.zeros(1, 1, 1025, 1024)),
               dict(scores=m, out=m), dict(scores=m, out=torch.empty(2, 3, 6, 6).double()), dict(scores=m, out=torch.empty(2, 2, 6, 6)),
               dict(scores=m, out=torch.empty(2, 3, 6, 12)[..., ::2]), dict(trans=trans, scores=m, out=trans[:, :3], radius=2),
               dict(scores=torch.zeros(2, 6, 6, 6)[:, :3], out=torch.zeros(0))):
        kw.setdefault("radius", 5)
        radius = kw.pop("radius")
        with pytest.raises(ops.WsdlError):
            ops.check_affinity_options(radius, **kw)
    flat = torch.zeros(2 * 3 * 6 * 6 + 216)
    with pytest.raises(ops.WsdlError, match="shares memory"):                # two dense views of one buffer that overlap
        ops.check_affinity_options(5, scores=flat[:216].view(2, 3, 6, 6), out=flat[5:221].view(2, 3, 6, 6))
    ops.check_affinity_options(5, scores=flat[:216].view(2, 3, 6, 6), out=flat[216:].view(2, 3, 6, 6))     # side by side: fine
    # host tensors never reach a kernel
    for call in (lambda: ops.pair_affinity(f), lambda: ops.affinity_loss(f, lab), lambda: ops.affinity_pair_counts(lab),
                 lambda: ops.random_walk(torch.zeros(2, 69, 6, 6), m, 2)):
        with pytest.raises(ops.WsdlError):
            call()
    assert ops.affinity_workspace(16, 448, 21, 32, 32, 5) > 0
    for geom in ((1, 1025, 1, 8, 8, 5), (1, 4, 33, 8, 8, 5), (1, 4, 1, 1025, 1024, 5), (1, 4, 1, 8, 8, 9), (0, 4, 1, 8, 8, 5)):
        assert ops.affinity_workspace(*geom) == 0


def test_modules_validate_on_the_host():
    from weaklysuperviseddl_amd import ops, nn as wnn
    crit, walk = wnn.AffinityLoss(), wnn.RandomWalk()
    assert (crit.radius, crit.ignore_index, crit.weights) == (5, 255, (0.25, 0.25, 0.5))
    assert (walk.radius, walk.beta, walk.num_iter) == (5, 8.0, 256)
    assert not isinstance(crit, wnn._Criterion) and not list(crit.parameters()) and not list(walk.parameters())
    for bad in (lambda: wnn.AffinityLoss(radius=1), lambda: wnn.AffinityLoss(weights=(1, 2)), lambda: wnn.RandomWalk(beta=0),
                lambda: wnn.RandomWalk(num_iter=-3), lambda: wnn.RandomWalk(radius=12)):
        with pytest.raises(ops.WsdlError):
            bad()


def test_generate_pseudo_masks_refuses_combinations():
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks
    import inspect
    assert inspect.signature(generate_pseudo_masks).parameters["affinity"].default is None
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, affinity={"net": object()}, pamr={})
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, affinity={"net": object()}, superpixels={"step": 8})
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, affinity={"radius": 5})                      # no net
    with pytest.raises(ValueError):
        generate_pseudo_masks([], None, affinity={"net": object(), "steps": 3})     # an unknown key
    with pytest.raises(ops.WsdlError):
        generate_pseudo_masks([], None, affinity={"net": object(), "radius": 11})


def test_affinity_net_parameters_and_labels():
    from weaklysuperviseddl_amd.TraditionalModel import AffinityNet, FrozenResNetCAM, affinity_labels_from_cam
    net = AffinityNet(FrozenResNetCAM(37))
    head = {k: tuple(p.shape) for k, p in net.named_parameters() if p.requires_grad}
    assert head == {"f8_3.weight": (64, 512, 1, 1), "f8_4.weight": (128, 1024, 1, 1), "f8_5.weight": (256, 2048, 1, 1),
                    "f9.weight": (448, 448, 1, 1)}
    assert all(k.startswith("trunk.") for k, p in net.named_parameters() if not p.requires_grad)
    assert len(net.head_parameters()) == 4 and not net.train().trunk.training and net.training
    cam = torch.linspace(0, 1, 64).view(1, 1, 64).expand(2, 64, 64).contiguous()
    cam[0, 0, 0] = float("nan")
    lab = affinity_labels_from_cam(cam, 0.25, 0.75, (8, 8))
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, 8, 8)
    # nearest: the sample of output column i is input column floor((i + 0.5) * 8) = 8 i + 4
    want = torch.where(cam[:, 4::8, 4::8] >= 0.75, 1, torch.where(cam[:, 4::8, 4::8] <= 0.25, 0, 255))
    assert torch.equal(lab, want) and set(lab.unique().tolist()) == {0, 1, 255}
    with pytest.raises(ValueError):
        affinity_labels_from_cam(cam, 0.5, 0.5, (8, 8))


def test_train_affinity_net_refuses_bad_options_on_the_host():
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import AffinityNet, FrozenResNetCAM, train_affinity_net
    net = AffinityNet(FrozenResNetCAM(37))
    cams = [torch.zeros(1, 8, 8)]
    for kw in (dict(epochs=0), dict(epochs=1.5), dict(lo=0.5, hi=0.5), dict(cams=3)):
        kw.setdefault("cams", cams)
        with pytest.raises(ValueError):
            train_affinity_net(net, [], log=None, **kw)
    with pytest.raises(ValueError):
        train_affinity_net(torch.nn.Linear(1, 1), [], cams, log=None)
    for kw in (dict(radius=9), dict(weights=(1, 2))):
        with pytest.raises(ops.WsdlError):
            train_affinity_net(net, [], cams, log=None, **kw)
    assert all(p.device.type == "cpu" for p in net.parameters())            # refused before anything moved


def test_out_without_its_tensor_is_refused():
    from weaklysuperviseddl_amd import ops
    with pytest.raises(ops.WsdlError):
        ops.check_affinity_options(5, out=torch.empty(1, 1, 2, 2))
