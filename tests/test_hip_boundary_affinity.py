"""IRN boundary-path affinities, their loss and the boundary CAM walk on the device (csrc/boundary_affinity.hip) against the
oracle of tests/boundary_affinity_oracle.py.

The affinities and their arg indices are exact: a maximum and one float subtraction, so the device must equal the float32 run
of the oracle BIT FOR BIT.  Everything else is under the project's standing parity bound: the SAME oracle run in torch float32 on
the CPU against its float64 run is the yardstick, computed here per case and never taken from the device; the device may be at
most ``max(4 x yardstick, 2^-23 |value|)`` away from float64 (maxima over the tensor).  The worst device-error-to-bound ratios
are reported with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_oracle as ao  # noqa: E402
import boundary_affinity_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
# (case, radius, beta, C)
WALK_CASES = ((3, 8, 10.0, 1), (4, 5, 10.0, 2))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def bound(yard, value):
    return max(4.0 * yard, ULP * value.abs().max().item())


def maxerr(a, b):
    return (a.detach().cpu().double() - b).abs().max().item()


def ratio(e, b):
    return e / b if b > 0 else (0.0 if e == 0 else float("inf"))


def name_of(case, radius):
    return "x".join(str(v) for v in bo.CASES[case]) + f" r={radius}"


def same_bits(a, b):
    """Equal where both are numbers, NaN exactly where the other is."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(b)
    return a.dtype == b.dtype and torch.equal(torch.isnan(a), nan) and torch.equal(a[~nan], b[~nan])


@functools.lru_cache(maxsize=None)
def affinity_reference(case, radius, content):
    """The float32 oracle of one (shape, radius, content): what the device must equal bit for bit."""
    B, h, w = bo.CASES[case]
    edge = bo.make_edge(B, h, w, 100 + case, content)
    a32, arg = bo.affinity(edge, radius, dtype=torch.float32)
    assert a32.dtype == torch.float32
    return dict(edge=edge, a32=a32, arg=arg.to(torch.uint8))


@functools.lru_cache(maxsize=None)
def backward_reference(case, radius):
    B, h, w = bo.CASES[case]
    edge = bo.make_edge(B, h, w, 100 + case)
    _, arg, valid = bo.path_max(edge, radius)
    daff = torch.randn(B, len(ao.offsets(radius)), h, w, generator=torch.Generator().manual_seed(400 + case))
    g64 = bo.affinity_backward(daff.double(), arg, valid, radius)
    g32 = bo.affinity_backward(daff, arg, valid, radius)
    assert g32.dtype == torch.float32
    return dict(edge=edge, daff=daff, g64=g64, yard=(g32.double() - g64).abs().max().item())


@functools.lru_cache(maxsize=None)
def loss_reference(case, radius, variant="all"):
    B, h, w = bo.CASES[case]
    logits = bo.make_logits(B, h, w, 100 + case)
    labels = ao.make_labels(B, h, w, 200 + case, variant)
    L64, g64 = bo.loss(logits, labels, radius)
    L32, g32 = bo.loss(logits, labels, radius, dtype=torch.float32)
    assert L32.dtype == torch.float32 and g32.dtype == torch.float32
    return dict(logits=logits, labels=labels, L64=L64, g64=g64, counts=ao.pair_counts(labels, radius),
                yard_L=abs(L32.double().item() - L64.item()), yard_g=(g32.double() - g64).abs().max().item())


@functools.lru_cache(maxsize=None)
def composed_reference(case, radius):
    """path_affinity followed by PSA's loss on the affinities: float64 and float32, the gradient by the explicit scatter."""
    B, h, w = bo.CASES[case]
    edge = bo.make_edge(B, h, w, 100 + case)
    labels = ao.make_labels(B, h, w, 200 + case)
    kinds = ao.pair_kinds(labels, radius)
    out = {}
    for dtype in (torch.float64, torch.float32):
        m, arg, valid = bo.path_max(edge, radius, dtype)
        aff = torch.where(valid, 1 - m, torch.zeros_like(m)).requires_grad_()
        L = ao.loss_from_affinity(aff, kinds)
        L.backward()
        out[dtype] = (L.detach(), bo.affinity_backward(aff.grad, arg, valid, radius))
    (L64, g64), (L32, g32) = out[torch.float64], out[torch.float32]
    assert g32.dtype == torch.float32
    return dict(edge=edge, kinds=kinds, L64=L64, g64=g64, yard_L=abs(L32.double().item() - L64.item()),
                yard_g=(g32.double() - g64).abs().max().item())


@functools.lru_cache(maxsize=None)
def walk_reference(i):
    case, radius, beta, C = WALK_CASES[i]
    B, h, w = bo.CASES[case]
    edge = bo.make_edge(B, h, w, 100 + case)
    scores = ao.make_scores(B, C, h, w, 300 + i)
    w64 = bo.edge_walk(edge, scores, radius, beta, bo.WALK_STEPS)
    w32 = bo.edge_walk(edge, scores, radius, beta, bo.WALK_STEPS, dtype=torch.float32)
    assert w32[1].dtype == torch.float32
    return dict(edge=edge, scores=scores, w64=w64, yard={n: (w32[n].double() - w64[n]).abs().max().item() for n in bo.WALK_STEPS})


@pytest.mark.parametrize("radius", bo.RADII)
@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_affinities_and_arg_indices_equal_the_float32_oracle_bit_for_bit(dev, case, radius):
    from weaklysuperviseddl_amd import ops
    for content in bo.CONTENTS:
        r = affinity_reference(case, radius, content)
        e = r["edge"].to(dev)
        aff, arg = ops.path_affinity(e, radius, return_arg=True)
        assert aff.dtype == torch.float32 and arg.dtype == torch.uint8 and aff.is_contiguous() and aff.grad_fn is None
        assert tuple(aff.shape) == tuple(r["a32"].shape) == tuple(arg.shape)
        assert torch.equal(aff.cpu(), r["a32"]), (content, (aff.cpu() - r["a32"]).abs().max().item())
        assert torch.equal(arg.cpu(), r["arg"]), content
        # the (B,1,h,w) form and the call without the arg plane: the same affinities; the input is untouched
        assert torch.equal(ops.path_affinity(e[:, None], radius), aff) and torch.equal(e.cpu(), r["edge"])


def test_no_valid_pair_at_all(dev):
    """1 x 1 x 1: affinities 0, loss 0, gradient 0, the walk returns the damped seed."""
    from weaklysuperviseddl_amd import ops
    e = torch.full((1, 1, 1), 0.25, device=dev, requires_grad=True)
    for radius in bo.RADII:
        assert not ops.path_affinity(e.detach(), radius).any()
        L = ops.path_affinity_loss(e, torch.ones(1, 1, 1, dtype=torch.int64, device=dev), radius=radius)
        (g,) = torch.autograd.grad(L, e)
        assert L.item() == 0.0 and g.item() == 0.0
        m = torch.tensor([0.5, -2.0], device=dev).view(1, 2, 1, 1)
        assert torch.equal(ops.edge_random_walk(e.detach(), m, radius=radius, num_iter=5), m * 0.75)


@pytest.mark.parametrize("radius", bo.RADII)
def test_nan_pixels_give_nan_where_the_oracle_has_it(dev, radius):
    from weaklysuperviseddl_amd import ops
    edge = bo.make_edge(2, 9, 11, 7)
    edge[0, 4, 5] = edge[0, 4, 6] = edge[1, 0, 0] = edge[1, 8, 10] = float("nan")
    a32, arg = bo.affinity(edge, radius, dtype=torch.float32)
    aff, darg = ops.path_affinity(edge.to(dev), radius, return_arg=True)
    assert torch.isnan(a32).any() and same_bits(aff, a32) and torch.equal(darg.cpu(), arg.to(torch.uint8))


@pytest.mark.parametrize("radius", bo.RADII)
@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_backward_of_the_affinities_against_float64(dev, case, radius):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = backward_reference(case, radius)
    e = r["edge"].to(dev).requires_grad_()
    aff = ops.path_affinity(e, radius)
    (g,) = torch.autograd.grad(aff, e, r["daff"].to(dev))
    err, b = maxerr(g, r["g64"]), bound(r["yard"], r["g64"])
    report_line(f"path affinity backward {name_of(case, radius)}: device error / bound {ratio(err, b):.2f}")
    print(f"{name_of(case, radius)}: {err:.3e} / bound {b:.3e}")
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(e.shape)
    assert err <= b, (err, b)


@pytest.mark.parametrize("case,radius", ((3, 5), (4, 5), (5, 8)))
def test_autograd_through_the_affinities_and_a_loss_on_them(dev, case, radius):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = composed_reference(case, radius)
    e = r["edge"].to(dev).requires_grad_()
    L = ao.loss_from_affinity(ops.path_affinity(e, radius), r["kinds"].to(dev))
    L.backward()
    e_L, e_g = abs(L.item() - r["L64"].item()), maxerr(e.grad, r["g64"])
    b_L, b_g = bound(r["yard_L"], r["L64"]), bound(r["yard_g"], r["g64"])
    report_line(f"path affinity + loss on it {name_of(case, radius)}: device error / bound: loss {ratio(e_L, b_L):.2f}, gradient "
                f"{ratio(e_g, b_g):.2f}")
    assert e_L <= b_L, (e_L, b_L)
    assert e_g <= b_g, (e_g, b_g)


@pytest.mark.parametrize("radius", bo.RADII)
@pytest.mark.parametrize("case", range(len(bo.CASES)))
def test_fused_loss_gradient_and_counts_against_float64(dev, case, radius):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = loss_reference(case, radius)
    z = r["logits"].to(dev).requires_grad_()
    counts = torch.full((3,), -1, dtype=torch.int64, device=dev)
    L = ops.path_affinity_loss(z, r["labels"].to(dev), radius=radius, counts_out=counts)
    L.backward()
    e_L, e_g = abs(L.item() - r["L64"].item()), maxerr(z.grad, r["g64"])
    b_L, b_g = bound(r["yard_L"], r["L64"]), bound(r["yard_g"], r["g64"])
    report_line(f"path affinity loss {name_of(case, radius)}: device error / bound: loss {ratio(e_L, b_L):.2f}, gradient {ratio(e_g, b_g):.2f}")
    print(f"{name_of(case, radius)}: L {e_L:.3e} / {b_L:.3e} (L = {r['L64'].item():.6f}); g {e_g:.3e} / {b_g:.3e}; counts "
          f"{r['counts'].tolist()}")
    assert L.dtype == torch.float32 and L.dim() == 0 and tuple(z.grad.shape) == tuple(z.shape) and z.grad.dtype == torch.float32
    assert counts.tolist() == r["counts"].tolist()
    assert torch.isfinite(L) and torch.isfinite(z.grad).all() and r["logits"].abs().max().item() == 40.0
    assert e_L <= b_L, (e_L, b_L)
    assert e_g <= b_g, (e_g, b_g)


@pytest.mark.parametrize("variant", ("no_bg", "ignored"))
@pytest.mark.parametrize("case,radius", ((3, 5), (4, 5), (5, 2)))
def test_loss_with_a_kind_absent_and_with_everything_ignored(dev, case, radius, variant):
    from weaklysuperviseddl_amd import ops
    r = loss_reference(case, radius, variant)
    z = r["logits"].to(dev).requires_grad_()
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    L = ops.path_affinity_loss(z, r["labels"].to(dev), radius=radius, counts_out=counts)
    L.backward()
    want = r["counts"].tolist()
    assert counts.tolist() == want
    if variant == "ignored":
        assert want == [0, 0, 0] and L.item() == 0.0 and not z.grad.any()
    else:
        assert want[0] == 0 and want[1] > 0 and want[2] > 0
    e_L, e_g = abs(L.item() - r["L64"].item()), maxerr(z.grad, r["g64"])
    assert e_L <= bound(r["yard_L"], r["L64"]), (e_L, r["yard_L"])
    assert e_g <= bound(r["yard_g"], r["g64"]), (e_g, r["yard_g"])


@pytest.mark.parametrize("case,radius", ((3, 8), (4, 5), (6, 2)))
def test_call_mechanics(dev, case, radius):
    """Two calls give the same bits, the inputs are never written, the incoming scalar scales the fused gradient, logits may
    be (B,1,h,w), and strided logits that need a gradient work on a dense copy."""
    from weaklysuperviseddl_amd import ops
    r = loss_reference(case, radius)
    lab = r["labels"].to(dev)
    z1, z2 = r["logits"].to(dev).requires_grad_(), r["logits"].to(dev).requires_grad_()
    L1, L2 = ops.path_affinity_loss(z1, lab, radius=radius), ops.path_affinity_loss(z2, lab, radius=radius)
    L1.backward()
    L2.backward()
    assert torch.equal(L1, L2) and torch.equal(z1.grad, z2.grad)
    assert torch.equal(z1.detach().cpu(), r["logits"]) and torch.equal(lab.cpu(), r["labels"])
    z3 = r["logits"].to(dev).requires_grad_()
    (ops.path_affinity_loss(z3, lab, radius=radius) * 0.5).backward()
    assert torch.equal(z3.grad, z1.grad * 0.5)
    z4 = r["logits"].to(dev)[:, None].requires_grad_()
    L4 = ops.path_affinity_loss(z4, lab, radius=radius)
    L4.backward()
    assert torch.equal(L4, L1) and torch.equal(z4.grad[:, 0], z1.grad)
    with torch.no_grad():
        assert torch.equal(ops.path_affinity_loss(z1, lab, radius=radius), L1)            # (no gradient buffer: the same loss)
    base = torch.stack([r["logits"], r["logits"]], dim=-1).to(dev).requires_grad_()
    view = base[..., 1]
    assert not view.is_contiguous() or view.numel() == 1
    ops.path_affinity_loss(view, lab, radius=radius).backward()
    assert torch.equal(base.grad[..., 1], z1.grad) and not base.grad[..., 0].any()
    e = affinity_reference(case, radius, "quantised")["edge"].to(dev)
    wide = torch.stack([e, e], dim=-1).requires_grad_()
    a1, a2 = ops.path_affinity(wide[..., 0], radius), ops.path_affinity(e, radius)
    assert torch.equal(a1, a2) and torch.equal(ops.path_affinity(e, radius), a2)
    a1.sum().backward()
    assert not wide.grad[..., 1].any() and wide.grad[..., 0].abs().sum().item() > 0


@pytest.mark.parametrize("i", range(len(WALK_CASES)))
def test_edge_random_walk_is_its_composition_and_meets_float64(dev, i):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    case, radius, beta, C = WALK_CASES[i]
    r = walk_reference(i)
    e, m = r["edge"].to(dev), r["scores"].to(dev)
    worst = 0.0
    for n in bo.WALK_STEPS:
        out = ops.edge_random_walk(e, m, radius=radius, beta=beta, num_iter=n)
        composed = ops.random_walk(ops.affinity_transitions(ops.path_affinity(e, radius), beta, radius), m * (1 - e[:, None]), n,
                                   radius=radius)
        assert torch.equal(out, composed) and out.dtype == torch.float32 and out.grad_fn is None and not out.requires_grad
        err, b = maxerr(out, r["w64"][n]), bound(r["yard"][n], r["w64"][n])
        print(f"{name_of(case, radius)} beta={beta} C={C} steps={n}: {err:.3e} / bound {b:.3e}")
        worst = max(worst, ratio(err, b))
        assert err <= b, (n, err, b)
    report_line(f"edge walk {name_of(case, radius)} beta={beta:g} C={C}: device error / bound after 1, 16, 256 steps at most {worst:.2f}")
    o = torch.full_like(m, float("nan"))
    assert ops.edge_random_walk(e[:, None], m, radius=radius, beta=beta, num_iter=16, out=o) is o
    assert torch.equal(o, ops.edge_random_walk(e, m, radius=radius, beta=beta, num_iter=16))
    assert torch.equal(e.cpu(), r["edge"]) and torch.equal(m.cpu(), r["scores"])


def test_a_column_of_one_stops_the_walk(dev):
    """Scores that are zero on one side of a full-height edge = 1 column are still exactly zero there after 256 steps."""
    from weaklysuperviseddl_amd import ops
    h, w, col = 20, 70, 33
    e = torch.rand(2, h, w, generator=torch.Generator().manual_seed(11)) * 0.5
    e[:, :, col] = 1.0
    m = torch.zeros(2, 2, h, w)
    m[..., :col] = torch.rand(2, 2, h, col, generator=torch.Generator().manual_seed(12)) + 0.5
    for radius in (2, 5, 8):
        aff = ops.path_affinity(e.to(dev), radius).cpu()
        a32, _ = bo.affinity(e, radius, dtype=torch.float32)
        assert torch.equal(aff, a32)
        out = ops.edge_random_walk(e.to(dev), m.to(dev), radius=radius, beta=10.0, num_iter=256)
        assert not out[..., col:].any() and out[..., :col].min().item() > 0


def test_modules_are_the_ops(dev):
    from weaklysuperviseddl_amd import ops, nn as wnn
    r = loss_reference(3, 5)
    z, lab = r["logits"].to(dev), r["labels"].to(dev)
    z1, z2 = z.clone().requires_grad_(), z.clone().requires_grad_()
    crit = wnn.PathAffinityLoss(5, 255, (0.3, 0.2, 0.5))
    L1, L2 = crit(z1, lab), ops.path_affinity_loss(z2, lab, radius=5, ignore_index=255, weights=(0.3, 0.2, 0.5))
    L1.backward()
    L2.backward()
    assert torch.equal(L1, L2) and torch.equal(z1.grad, z2.grad)
    assert not torch.equal(L1, ops.path_affinity_loss(z, lab))          # (the weights matter)
    e = bo.make_edge(2, 5, 7, 1).to(dev)
    m = ao.make_scores(2, 3, 5, 7, 1).to(dev)
    assert torch.equal(wnn.EdgeRandomWalk(2, 4.0, 9)(e, m), ops.edge_random_walk(e, m, radius=2, beta=4.0, num_iter=9))
    assert not isinstance(crit, wnn._Criterion)


def test_refusals_on_the_device(dev):
    from weaklysuperviseddl_amd import ops
    e, m = torch.rand(1, 8, 8, device=dev), torch.rand(1, 2, 8, 8, device=dev)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64, device=dev)
    for bad in (lambda: ops.path_affinity(e, 9), lambda: ops.path_affinity(e.cpu(), 5), lambda: ops.path_affinity(e.double(), 5),
                lambda: ops.path_affinity(torch.rand(1, 2, 8, 8, device=dev)), lambda: ops.path_affinity_loss(e, lab[:, :, :7]),
                lambda: ops.path_affinity_loss(e, lab.float()), lambda: ops.path_affinity_loss(e, lab.cpu()),
                lambda: ops.path_affinity_loss(e, lab, counts_out=torch.zeros(3, device=dev)),
                lambda: ops.edge_random_walk(e, torch.rand(1, 33, 8, 8, device=dev)), lambda: ops.edge_random_walk(e, m, out=m),
                lambda: ops.edge_random_walk(e, m[:, :1], out=e[:, None]), lambda: ops.edge_random_walk(e, m, num_iter=-1),
                lambda: ops.edge_random_walk(e, m, beta=0.0), lambda: ops.edge_random_walk(e, torch.rand(1, 2, 8, 9, device=dev))):
        with pytest.raises(ops.WsdlError):
            bad()


def test_launch_plans_replay_loss_and_walk(dev):
    from weaklysuperviseddl_amd import ops, plan
    r = loss_reference(4, 5)
    z, lab = r["logits"].to(dev).requires_grad_(), r["labels"].to(dev)

    def step():
        L = ops.path_affinity_loss(z, lab, radius=5)
        return L, torch.autograd.grad(L, z)[0]
    p, (L, g) = plan.record(step)
    eager_L, eager_g = step()
    assert torch.equal(L, eager_L) and torch.equal(g, eager_g)
    with torch.no_grad():
        z.copy_((z * 0.5 + 0.25 * z.flip(-1)).contiguous())
        lab.copy_(lab.flip(-1).contiguous())
    p.replay()
    torch.cuda.synchronize()
    rep_L, rep_g = L.clone(), g.clone()
    new_L, new_g = step()
    assert torch.equal(rep_L, new_L) and torch.equal(rep_g, new_g) and not torch.equal(rep_g, eager_g)

    w = walk_reference(1)
    e, m = w["edge"].to(dev), w["scores"].to(dev)
    o = torch.empty_like(m)

    def walk():
        return ops.edge_random_walk(e, m, radius=5, beta=10.0, num_iter=6, out=o)
    p2, res = plan.record(walk)
    # the seed, the affinities, the transitions and six steps
    assert res is o and p2.stats["kernels"] == 9 and torch.equal(o, walk().clone())
    first = o.clone()
    e.copy_((e * 0.7).contiguous())
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


def test_boundary_net_and_generate_pseudo_masks(dev):
    """A 64 x 64 image through BoundaryNet: finite logits (B,1,16,16), finite non-zero gradients on the six head convolutions
    only.  generate_pseudo_masks(boundary=None) is the call without the argument, bit for bit, and with a net it equals the
    composition of the ops."""
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import BoundaryNet, affinity_labels_from_cam, generate_pseudo_masks
    model, gen = _cam_generator(dev)
    torch.manual_seed(1)
    net = BoundaryNet(model).to(dev).train()
    assert not net.trunk.training
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    logits = net(x)
    assert tuple(logits.shape) == (2, 1, 16, 16) and torch.isfinite(logits).all()
    cam = torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    labels = affinity_labels_from_cam(cam, 0.3, 0.6, logits.shape[-2:])
    assert tuple(labels.shape) == (2, 16, 16) and set(labels.unique().tolist()) <= {0, 1, 255}
    ops.path_affinity_loss(logits, labels, radius=5).backward()
    with_grad = sorted(k for k, p in net.named_parameters() if p.grad is not None)
    assert with_grad == ["fc_edge1.weight", "fc_edge2.weight", "fc_edge3.weight", "fc_edge4.weight", "fc_edge5.weight", "fc_edge6.bias",
                         "fc_edge6.weight"]
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, k

    net.eval()
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 224, 224, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_pseudo_masks(loader, gen, boundary=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    generate_pseudo_masks(loader, gen, boundary=dict(net=net, radius=3, beta=4.0, num_iter=8), **kw)
    walked = torch.stack(generate_pseudo_masks.last_masks)
    imgs = loader[0][0].to(dev)
    cam, _ = gen.generate_batch(imgs, alpha=1.0, class_idx=loader[0][1][0].to(dev), thresh=0.3)
    with torch.no_grad():
        edge = torch.sigmoid(net(imgs))
    small = ops.bilinear_resize(cam[:, None].contiguous(), (56, 56))
    back = ops.bilinear_resize(ops.edge_random_walk(edge, small, radius=3, beta=4.0, num_iter=8), (224, 224))[:, 0]
    back = back / (back.amax(dim=(-2, -1), keepdim=True) + 1e-5)
    want = ops.keep_largest_batched((back >= 0.3).to(torch.uint8))
    assert tuple(edge.shape) == (2, 1, 56, 56) and torch.equal(walked, want) and walked.dtype == torch.uint8


def test_train_boundary_net_takes_steps(dev):
    """Two batches of 64 x 64 images, one epoch: the steps run and return a finite loss, every head parameter has a finite
    gradient, the trunk does not move.  Nothing is asked of the loss value: with -log(a + eps) it may even be slightly negative
    (a = 1 gives -log(1 + eps)), and a randomly initialised head without IRN's GroupNorm may start saturated, where the
    gradients are too small to move a float32 weight in two steps."""
    import math
    from weaklysuperviseddl_amd.TraditionalModel import BoundaryNet, train_boundary_net
    model, _ = _cam_generator(dev)
    torch.manual_seed(2)
    net = BoundaryNet(model)
    before = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
    g = torch.Generator().manual_seed(8)
    loader = [(torch.rand(2, 3, 64, 64, generator=g), None) for _ in range(2)]
    ramp = torch.linspace(0, 1, 64).view(1, 1, 64).expand(2, 64, 64).contiguous()
    history = train_boundary_net(net, loader, [ramp, ramp.transpose(1, 2).contiguous()], lo=0.45, hi=0.55, radius=5, device=dev, log=None)
    assert len(history) == 1 and math.isfinite(history[0]) and not net.training
    moved = [k for k, p in net.named_parameters() if not torch.equal(p.detach().cpu(), before[k])]
    print(f"loss {history[0]:.6e}; moved: {moved}")
    assert not any(k.startswith("trunk.") for k in moved)
    for k, p in net.named_parameters():
        if not k.startswith("trunk."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
