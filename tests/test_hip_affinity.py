"""AffinityNet affinities, their loss and the CAM random walk on the device (csrc/affinity.hip) against the float64 oracle of
tests/affinity_oracle.py.

Parity bound (the project's standing rule): the SAME oracle run in torch float32 on the CPU against its float64 run is the
yardstick, computed here per case and never taken from the device; the device may be at most ``max(4 x yardstick, 2^-23
|value|)`` away from float64 (maxima over the tensor).  The 4 x covers a different summation order over up to 448 or 193
terms and a different ``exp`` / ``log``; a walk step is a convex combination, so errors do not compound.  The worst
device-error-to-bound ratios are reported with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_oracle as ao  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def bound(yard, value):
    return max(4.0 * yard, ULP * value.abs().max().item())


def maxerr(a, b):
    return (a.detach().cpu().double() - b).abs().max().item()


@functools.lru_cache(maxsize=None)
def reference(case, radius, variant="all"):
    """Inputs, the float64 oracle and the float32 yardsticks of one (shape, radius, label variant) - computed once, shared,
    never written."""
    B, D, h, w = ao.CASES[case]
    feat = ao.make_features(B, D, h, w, 100 + case)
    labels = ao.make_labels(B, h, w, 200 + case, variant)
    a64, a32 = ao.affinity(feat, radius), ao.affinity(feat, radius, dtype=torch.float32)
    L64, g64 = ao.loss(feat, labels, radius)
    L32, g32 = ao.loss(feat, labels, radius, dtype=torch.float32)
    assert a32.dtype == torch.float32 and g32.dtype == torch.float32
    return dict(feat=feat, labels=labels, a64=a64, L64=L64, g64=g64, counts=ao.pair_counts(labels, radius),
                yard_a=(a32.double() - a64).abs().max().item(), yard_L=abs(L32.double().item() - L64.item()),
                yard_g=(g32.double() - g64).abs().max().item())


@functools.lru_cache(maxsize=None)
def walk_reference(i):
    case, radius, beta, C = ao.WALK_CASES[i]
    B, D, h, w = ao.CASES[case]
    feat = ao.make_features(B, D, h, w, 100 + case)
    scores = ao.make_scores(B, C, h, w, 300 + i)
    t64 = ao.transitions(ao.affinity(feat, radius), beta, radius)
    t32 = ao.transitions(ao.affinity(feat, radius, dtype=torch.float32), beta, radius)
    w64, w32 = ao.walk(t64, scores, ao.WALK_STEPS, radius), ao.walk(t32, scores, ao.WALK_STEPS, radius)
    assert t32.dtype == torch.float32 and w32[1].dtype == torch.float32
    return dict(feat=feat, scores=scores, radius=radius, beta=beta, t64=t64, w64=w64,
                yard_t=(t32.double() - t64).abs().max().item(),
                yard_w={n: (w32[n].double() - w64[n]).abs().max().item() for n in ao.WALK_STEPS})


def name_of(case, radius):
    return "x".join(str(v) for v in ao.CASES[case]) + f" r={radius}"


@pytest.mark.parametrize("radius", ao.RADII)
@pytest.mark.parametrize("case", range(len(ao.CASES)))
def test_affinities_loss_gradient_and_counts_against_float64(dev, case, radius):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = reference(case, radius)
    f = r["feat"].to(dev).requires_grad_()
    lab = r["labels"].to(dev)
    a = ops.pair_affinity(f.detach(), radius)
    L = ops.affinity_loss(f, lab, radius=radius)
    L.backward()
    counts = ops.affinity_pair_counts(lab, radius)
    e_a, e_L, e_g = maxerr(a, r["a64"]), abs(L.item() - r["L64"].item()), maxerr(f.grad, r["g64"])
    b_a, b_L, b_g = bound(r["yard_a"], r["a64"]), bound(r["yard_L"], r["L64"]), bound(r["yard_g"], r["g64"])
    ratio = lambda e, b: e / b if b > 0 else 0.0  # noqa: E731
    report_line(f"affinity {name_of(case, radius)}: device error / bound: affinities {ratio(e_a, b_a):.2f}, loss {ratio(e_L, b_L):.2f}, "
                f"gradient {ratio(e_g, b_g):.2f}")
    print(f"{name_of(case, radius)}: a {e_a:.3e} / bound {b_a:.3e}; L {e_L:.3e} / {b_L:.3e} (L = {r['L64'].item():.6f}); "
          f"g {e_g:.3e} / {b_g:.3e}; counts {r['counts'].tolist()}")
    assert tuple(a.shape) == tuple(r["a64"].shape) and a.dtype == torch.float32 and a.is_contiguous()
    assert L.dtype == torch.float32 and L.dim() == 0 and tuple(f.grad.shape) == tuple(f.shape)
    assert counts.dtype == torch.int64 and counts.tolist() == r["counts"].tolist()
    assert torch.equal(a.cpu() == 0, r["a64"] == 0)               # an invalid pair is exactly 0, a valid one is not
    assert e_a <= b_a, (e_a, b_a)
    assert e_L <= b_L, (e_L, b_L)
    assert e_g <= b_g, (e_g, b_g)


@pytest.mark.parametrize("variant", ("no_bg", "ignored"))
@pytest.mark.parametrize("case,radius", ((3, 5), (4, 5), (5, 2)))
def test_loss_with_a_kind_absent_and_with_everything_ignored(dev, case, radius, variant):
    from weaklysuperviseddl_amd import ops
    r = reference(case, radius, variant)
    f = r["feat"].to(dev).requires_grad_()
    L = ops.affinity_loss(f, r["labels"].to(dev), radius=radius)
    L.backward()
    counts = r["counts"].tolist()
    assert ops.affinity_pair_counts(r["labels"].to(dev), radius).tolist() == counts
    if variant == "ignored":
        assert counts == [0, 0, 0] and L.item() == 0.0 and not f.grad.any()
    else:
        assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0
    e_L, e_g = abs(L.item() - r["L64"].item()), maxerr(f.grad, r["g64"])
    assert e_L <= bound(r["yard_L"], r["L64"]), (e_L, r["yard_L"])
    assert e_g <= bound(r["yard_g"], r["g64"]), (e_g, r["yard_g"])


def test_no_valid_pair_at_all(dev):
    """1 x 1 x 1 x 1: affinities 0, loss 0, gradient 0, the walk is the identity."""
    from weaklysuperviseddl_amd import ops
    f = torch.full((1, 1, 1, 1), 0.7, device=dev, requires_grad=True)
    for radius in ao.RADII:
        assert not ops.pair_affinity(f.detach(), radius).any()
        L = ops.affinity_loss(f, torch.ones(1, 1, 1, dtype=torch.int64, device=dev), radius=radius)
        L.backward()
        assert L.item() == 0.0 and f.grad.item() == 0.0
        m = torch.tensor([0.3, -2.0], device=dev).view(1, 2, 1, 1)
        assert torch.equal(ops.affinity_random_walk(f.detach(), m, radius=radius, num_iter=5), m)


@pytest.mark.parametrize("i", range(len(ao.WALK_CASES)))
def test_transitions_and_walk_against_float64(dev, i):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    case, radius, beta, C = ao.WALK_CASES[i]
    r = walk_reference(i)
    f, m = r["feat"].to(dev), r["scores"].to(dev)
    trans = ops.affinity_transitions(ops.pair_affinity(f, radius), beta, radius)
    e_t, b_t = maxerr(trans, r["t64"]), bound(r["yard_t"], r["t64"])
    assert tuple(trans.shape) == tuple(r["t64"].shape) and trans.dtype == torch.float32
    assert (trans.sum(dim=1) - 1).abs().max().item() < 1e-6
    assert e_t <= b_t, (e_t, b_t)
    worst = 0.0
    for n in ao.WALK_STEPS:
        out = ops.random_walk(trans, m, n, radius=radius)
        e, b = maxerr(out, r["w64"][n]), bound(r["yard_w"][n], r["w64"][n])
        print(f"{name_of(case, radius)} beta={beta} C={C} steps={n}: {e:.3e} / bound {b:.3e}")
        worst = max(worst, e / b)
        assert out.dtype == torch.float32 and out.grad_fn is None and not out.requires_grad
        assert e <= b, (n, e, b)
        # a convex combination: inside the input's range
        assert out.min().item() >= m.min().item() - 1e-6 and out.max().item() <= m.max().item() + 1e-6
        assert torch.equal(ops.affinity_random_walk(f, m, radius=radius, beta=beta, num_iter=n), out)
    report_line(f"walk {name_of(case, radius)} beta={beta:g} C={C}: device error / bound: transitions {e_t / b_t:.2f}, scores after "
                f"1, 16, 256 steps at most {worst:.2f}")
    const = torch.full_like(m, 0.625)
    assert (ops.random_walk(trans, const, 256, radius=radius) - 0.625).abs().max().item() < 1e-6


@pytest.mark.parametrize("case,radius", ((3, 8), (5, 5), (2, 2)))
def test_zero_features_give_the_box_average(dev, case, radius):
    """Features x 0: every valid affinity is exactly 1 and a step is the plain average over the valid neighbours and the
    pixel itself."""
    from weaklysuperviseddl_amd import ops
    B, D, h, w = ao.CASES[case]
    f = torch.zeros(B, D, h, w, device=dev)
    a = ops.pair_affinity(f, radius)
    valid = ao.affinity(torch.zeros(B, D, h, w), radius) > 0
    assert torch.equal(a.cpu(), valid.float())
    m = ao.make_scores(B, 3, h, w, 9)
    ones = ao.transitions(valid.double(), 1.0, radius)
    want = ao.walk(ones, m, (1,), radius)[1]
    for beta in (1.0, 8.0):
        got = ops.affinity_random_walk(f, m.to(dev), radius=radius, beta=beta, num_iter=1)
        assert maxerr(got, want) <= 2e-7


@pytest.mark.parametrize("i", (3, 8, 11))
def test_call_mechanics(dev, i):
    """``out=`` reuse, every parity of num_iter, split step counts, a second call, untouched inputs, a strided view: the same
    bits.  (Only one walk path ships - the single-launch one was measured and dropped - so there is no second path to compare.)"""
    from weaklysuperviseddl_amd import ops
    case, radius, beta, C = ao.WALK_CASES[i]
    r = walk_reference(i)
    f, m = r["feat"].to(dev), r["scores"].to(dev)
    trans = ops.affinity_transitions(ops.pair_affinity(f, radius), beta, radius)
    t0, m0 = trans.clone(), m.clone()
    full = ops.random_walk(trans, m, 7, radius=radius)
    assert torch.equal(ops.random_walk(trans, m, 7, radius=radius), full)
    assert torch.equal(ops.random_walk(trans, ops.random_walk(trans, m, 3, radius=radius), 4, radius=radius), full)
    prev = m
    for n in (0, 1, 2, 3, 4):
        o = torch.full_like(m, float("nan"))
        got = ops.random_walk(trans, m, n, radius=radius, out=o)
        assert got is o and not torch.isnan(o).any()
        if n == 0:
            assert torch.equal(o, m)
        else:
            assert torch.equal(o, ops.random_walk(trans, prev, 1, radius=radius)), n
        prev = o
    # every channel equals its own one-channel run
    for c in range(0, C, 5):
        assert torch.equal(full[:, c:c + 1], ops.random_walk(trans, m[:, c:c + 1], 7, radius=radius)), c
    assert torch.equal(trans, t0) and torch.equal(m, m0)          # the inputs are never written
    tout = torch.full_like(trans, float("nan"))
    assert ops.affinity_transitions(ops.pair_affinity(f, radius), beta, radius, out=tout) is tout and torch.equal(tout, trans)
    # a strided view of the scores (channel slice of a wider tensor) and requires_grad inputs are accepted, detached
    wide = torch.cat([m, m], dim=1)[:, 1:1 + C].requires_grad_()
    res = ops.random_walk(trans, wide, 2, radius=radius)
    assert res.grad_fn is None and torch.equal(res, ops.random_walk(trans, wide.detach().contiguous(), 2, radius=radius))
    # two calls of the loss: identical bits
    lab = ao.make_labels(*[ao.CASES[case][k] for k in (0, 2, 3)], 7).to(dev)
    f1, f2 = f.clone().requires_grad_(), f.clone().requires_grad_()
    L1, L2 = ops.affinity_loss(f1, lab, radius=radius), ops.affinity_loss(f2, lab, radius=radius)
    L1.backward()
    L2.backward()
    assert torch.equal(L1, L2) and torch.equal(f1.grad, f2.grad) and torch.equal(f, r["feat"].to(dev))
    # the incoming scalar scales the fused gradient
    f3 = f.clone().requires_grad_()
    (ops.affinity_loss(f3, lab, radius=radius) * 0.5).backward()
    assert torch.equal(f3.grad, f1.grad * 0.5)


def test_refusals_on_the_device(dev):
    from weaklysuperviseddl_amd import ops
    f, m = torch.rand(1, 4, 8, 8, device=dev), torch.rand(1, 2, 8, 8, device=dev)
    trans = ops.affinity_transitions(ops.pair_affinity(f, 2), 8.0, 2)
    for bad in (lambda: ops.pair_affinity(f, 9), lambda: ops.pair_affinity(f.cpu(), 5), lambda: ops.pair_affinity(f.double(), 5),
                lambda: ops.random_walk(trans, torch.rand(1, 33, 8, 8, device=dev), 2, radius=2),
                lambda: ops.random_walk(trans, torch.rand(1, 2, 8, 9, device=dev), 2, radius=2),
                lambda: ops.random_walk(trans, m, 2, radius=5), lambda: ops.random_walk(trans, m, 2, radius=2, out=m),
                lambda: ops.random_walk(trans, m, -1, radius=2), lambda: ops.affinity_transitions(trans, 8.0, 2),
                lambda: ops.affinity_loss(f, torch.zeros(1, 8, 9, dtype=torch.int64, device=dev)),
                lambda: ops.affinity_loss(f, torch.zeros(1, 8, 8, device=dev)),
                lambda: ops.affinity_random_walk(torch.rand(1, 1025, 2, 2, device=dev), torch.rand(1, 1, 2, 2, device=dev))):
        with pytest.raises(ops.WsdlError):
            bad()


@pytest.mark.parametrize("case,radius", ((3, 5), (4, 5), (5, 8)))
def test_autograd_of_pair_affinity_equals_the_fused_gradient(dev, case, radius):
    from weaklysuperviseddl_amd import ops
    r = reference(case, radius)
    lab = r["labels"].to(dev)
    f1, f2 = r["feat"].to(dev).requires_grad_(), r["feat"].to(dev).requires_grad_()
    fused = ops.affinity_loss(f1, lab, radius=radius)
    fused.backward()
    composed = ao.loss_from_affinity(ops.pair_affinity(f2, radius), ao.pair_kinds(r["labels"], radius).to(dev))
    composed.backward()
    e = (f1.grad - f2.grad).abs().max().item()
    assert e <= bound(r["yard_g"], r["g64"]), (e, r["yard_g"])
    assert abs(fused.item() - composed.item()) <= bound(r["yard_L"], r["L64"])


def test_modules_are_the_ops(dev):
    from weaklysuperviseddl_amd import ops, nn as wnn
    r = reference(3, 5)
    f, lab = r["feat"].to(dev), r["labels"].to(dev)
    f1, f2 = f.clone().requires_grad_(), f.clone().requires_grad_()
    crit = wnn.AffinityLoss(5, 255, (0.3, 0.2, 0.5))
    L1, L2 = crit(f1, lab), ops.affinity_loss(f2, lab, radius=5, ignore_index=255, weights=(0.3, 0.2, 0.5))
    L1.backward()
    L2.backward()
    assert torch.equal(L1, L2) and torch.equal(f1.grad, f2.grad)
    assert not torch.equal(L1, ops.affinity_loss(f, lab))          # (the weights matter)
    m = ao.make_scores(2, 3, 5, 7, 1).to(dev)
    assert torch.equal(wnn.RandomWalk(2, 4.0, 9)(f, m), ops.affinity_random_walk(f, m, radius=2, beta=4.0, num_iter=9))
    assert not isinstance(crit, wnn._Criterion)


def test_launch_plans_replay_loss_and_walk(dev):
    from weaklysuperviseddl_amd import ops, plan
    r = reference(4, 5)
    f, lab = r["feat"].to(dev).requires_grad_(), r["labels"].to(dev)

    def step():
        L = ops.affinity_loss(f, lab, radius=5)
        return L, torch.autograd.grad(L, f)[0]
    p, (L, g) = plan.record(step)
    eager_L, eager_g = step()
    assert torch.equal(L, eager_L) and torch.equal(g, eager_g)
    with torch.no_grad():
        f.copy_((f * 0.5 + 0.25 * f.flip(-1)).contiguous())
        lab.copy_(lab.flip(-1).contiguous())
    p.replay()
    torch.cuda.synchronize()
    rep_L, rep_g = L.clone(), g.clone()
    new_L, new_g = step()
    assert torch.equal(rep_L, new_L) and torch.equal(rep_g, new_g) and not torch.equal(rep_g, eager_g)

    w = walk_reference(5)
    fw, m = w["feat"].to(dev), w["scores"].to(dev)
    o = torch.empty_like(m)

    def walk():
        return ops.random_walk(ops.affinity_transitions(ops.pair_affinity(fw, 5), 8.0, 5), m, 6, radius=5, out=o)
    p2, res = plan.record(walk)
    assert res is o and p2.stats["kernels"] == 8 and torch.equal(o, walk().clone())
    first = o.clone()
    fw.copy_((fw * 0.7).contiguous())
    m.copy_((1 - m).contiguous())
    p2.replay()
    torch.cuda.synchronize()
    replayed = o.clone()
    assert torch.equal(replayed, walk()) and not torch.equal(replayed, first)


def _cam_generator(dev):
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM, LayerCAMGenerator
    torch.manual_seed(0)
    model = FrozenResNetCAM(37)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    model = model.to(dev).eval()
    return model, LayerCAMGenerator(model, ["layer3", "layer4"])


def test_affinity_net_and_generate_pseudo_masks(dev):
    """A 64 x 64 image through AffinityNet: finite features of the documented shape, finite non-zero gradients on the four head
    convolutions only.  generate_pseudo_masks(affinity=None) is the call without the argument, bit for bit, and with a net it
    equals the composition of the ops."""
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import AffinityNet, affinity_labels_from_cam, generate_pseudo_masks
    model, gen = _cam_generator(dev)
    torch.manual_seed(1)
    net = AffinityNet(model).to(dev).train()
    assert not net.trunk.training
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    feat = net(x)
    assert tuple(feat.shape) == (2, 448, 8, 8) and torch.isfinite(feat).all()
    cam = torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    labels = affinity_labels_from_cam(cam, 0.3, 0.6, feat.shape[-2:])
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (2, 8, 8) and set(labels.unique().tolist()) <= {0, 1, 255}
    ops.affinity_loss(feat, labels, radius=5).backward()
    with_grad = sorted(k for k, p in net.named_parameters() if p.grad is not None)
    assert with_grad == ["f8_3.weight", "f8_4.weight", "f8_5.weight", "f9.weight"]
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, k

    net.eval()
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 224, 224, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_pseudo_masks(loader, gen, affinity=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    generate_pseudo_masks(loader, gen, affinity=dict(net=net, radius=3, beta=4.0, num_iter=8), **kw)
    walked = torch.stack(generate_pseudo_masks.last_masks)
    imgs = loader[0][0].to(dev)
    cam, _ = gen.generate_batch(imgs, alpha=1.0, class_idx=loader[0][1][0].to(dev), thresh=0.3)
    with torch.no_grad():
        ft = net(imgs)
    small = ops.bilinear_resize(cam[:, None].contiguous(), (28, 28))
    back = ops.bilinear_resize(ops.affinity_random_walk(ft, small, radius=3, beta=4.0, num_iter=8), (224, 224))[:, 0]
    want = ops.keep_largest_batched((back >= 0.3).to(torch.uint8))
    assert tuple(ft.shape) == (2, 448, 28, 28) and torch.equal(walked, want) and walked.dtype == torch.uint8


def test_strided_features_that_need_a_gradient(dev):
    """Non-contiguous features: the ops work on a dense copy, the gradient still reaches the argument."""
    from weaklysuperviseddl_amd import ops
    r = reference(3, 5)
    f, lab = r["feat"].to(dev), r["labels"].to(dev)
    base = torch.cat([f, f], dim=1).requires_grad_()
    view = base[:, 1:1 + f.shape[1]]
    assert not view.is_contiguous()
    ops.affinity_loss(view, lab, radius=5).backward()
    ref = view.detach().contiguous().requires_grad_()
    ops.affinity_loss(ref, lab, radius=5).backward()
    assert torch.equal(base.grad[:, 1:1 + f.shape[1]], ref.grad) and not base.grad[:, 0].any()


def test_infinite_scores_spread_as_infinity(dev):
    """A neighbour outside the image contributes neither its weight nor any score: inf at a border pixel stays inf (0 x inf
    would be NaN)."""
    from weaklysuperviseddl_amd import ops
    f = ao.make_features(1, 3, 6, 7, 2).to(dev)
    m = ao.make_scores(1, 2, 6, 7, 3).to(dev)
    m[0, 0, 0, 0] = float("inf")
    out = ops.affinity_random_walk(f, m, radius=3, beta=1.0, num_iter=2)
    assert not torch.isnan(out).any() and torch.isinf(out[0, 0, 0, 0]) and torch.isfinite(out[0, 1]).all()


def test_train_affinity_net_takes_steps(dev):
    """Two batches of 64 x 64 images, one epoch: a finite loss, the four head convolutions move, the trunk does not."""
    from weaklysuperviseddl_amd.TraditionalModel import AffinityNet, train_affinity_net
    model, _ = _cam_generator(dev)
    torch.manual_seed(2)
    net = AffinityNet(model)
    before = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
    g = torch.Generator().manual_seed(8)
    loader = [(torch.rand(2, 3, 64, 64, generator=g), None) for _ in range(2)]
    ramp = torch.linspace(0, 1, 64).view(1, 1, 64).expand(2, 64, 64).contiguous()
    history = train_affinity_net(net, loader, [ramp, ramp.transpose(1, 2).contiguous()], lo=0.3, hi=0.6, radius=3, device=dev, log=None)
    assert len(history) == 1 and history[0] == history[0] and 0 < history[0] < float("inf") and not net.training
    for k, p in net.named_parameters():
        same = torch.equal(p.detach().cpu(), before[k])
        assert same == k.startswith("trunk."), k
