"""Class prototypes, prototype similarity, the pixel-to-prototype contrast loss and the prototype bank on the device
(csrc/prototype.hip) against the float64 oracle of tests/prototype_oracle.py.

Parity bound (the project's standing rule): the SAME oracle run in torch float32 on the CPU against its float64 run is the
yardstick, computed here per case and never taken from the device; the device may be at most ``max(4 x yardstick, 2^-23
|value|)`` away from float64 (maxima over the tensor).  No extra term is needed: the kernels sum in double, so what separates
them from float64 is the rounding of a stored float (2^-24 of the value) and, for the mean's gradient, the float factor ``1 /
sum w`` and the float product with it (two more roundings) - below what the float32 oracle's own chain of a dozen rounded
operations per value leaves.  Every comparison feeds the device the float32 inputs the oracle was given (prototypes included:
the similarity and the loss are tested on the oracle's prototypes, so pooling errors do not enter them).  The worst
device-error-to-bound ratios are reported with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prototype_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23

# (case of po.CASES, K, per_image, temperature, index into po.OFFSETS): every shape with classes on both sides of a bucket, both
# segmentations, every temperature and both feature offsets
PARAMS = ((0, 1, True, 1.0, 0), (0, 2, False, 0.1, 1), (1, 2, True, 0.07, 0), (2, 3, False, 0.1, 0), (3, 3, True, 0.1, 1),
          (3, 21, False, 0.07, 0), (3, 32, True, 1.0, 0), (4, 21, True, 0.1, 0), (4, 2, False, 0.07, 1), (5, 32, True, 0.1, 0),
          (5, 2, False, 1.0, 1), (6, 3, True, 0.07, 1), (6, 21, False, 0.1, 0), (7, 2, True, 0.1, 0), (7, 32, False, 0.07, 0),
          (8, 1, False, 0.1, 0), (8, 3, True, 1.0, 1), (8, 21, True, 0.07, 0),
          # both sides of the per-pixel kernels' 24-class bucket and of the 16 | 32 boundary of the pool kernel
          (3, 16, True, 0.1, 0), (3, 17, False, 0.1, 0), (3, 24, True, 0.07, 0), (3, 25, False, 0.1, 0), (3, 4, True, 0.1, 0),
          (3, 5, False, 0.1, 0), (3, 8, True, 0.1, 0), (3, 9, False, 0.1, 0))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def bound(yard, value):
    return max(4.0 * yard, ULP * value.abs().max().item())


def maxerr(a, b):
    return (a.detach().cpu().double() - b).abs().max().item()


def yard(a32, a64):
    assert a32.dtype == torch.float32
    return (a32.double() - a64).abs().max().item()


def name_of(i):
    case, K, per_image, T, off = PARAMS[i]
    return "x".join(str(v) for v in po.CASES[case]) + f" K={K} S={'B' if per_image else 1} T={T} offset={po.OFFSETS[off][0]:g}"


@functools.lru_cache(maxsize=None)
def reference(i, variant="all", eps=1e-12):
    """Inputs, the float64 oracle and the float32 yardsticks of one entry of PARAMS - computed once, shared, never written."""
    case, K, per_image, T, off = PARAMS[i]
    B, D, h, w = po.CASES[case]
    feat = po.make_features(B, D, h, w, 100 + i, *po.OFFSETS[off])
    labels = po.make_labels(B, h, w, K, 200 + i, variant)
    pw = po.make_weights(B, h, w, 300 + i)
    r = dict(feat=feat, labels=labels, pw=pw, K=K, per_image=per_image, T=T, eps=eps)
    for tag, weights in (("", None), ("_w", pw)):
        p64, m64 = po.prototypes(feat, labels, K, weights, per_image, eps=eps)
        p32, m32 = po.prototypes(feat, labels, K, weights, per_image, eps=eps, dtype=torch.float32)
        r.update({"p64" + tag: p64, "m64" + tag: m64, "yard_p" + tag: yard(p32, p64), "yard_m" + tag: yard(m32, m64)})
    r["raw64"], _ = po.prototypes(feat, labels, K, None, per_image, normalize=False)
    r["yard_raw"] = yard(po.prototypes(feat, labels, K, None, per_image, normalize=False, dtype=torch.float32)[0], r["raw64"])
    proto = r["p64"].float()                                   # what the device is given: the oracle's prototypes, rounded
    present = r["m64"] > 0
    r.update(proto=proto, present=present)
    for act in ("none", "relu", "softmax"):
        s64 = po.similarity(feat, proto, act, T, present, eps)
        r["s64_" + act] = s64
        r["yard_s_" + act] = yard(po.similarity(feat, proto, act, T, present, eps, dtype=torch.float32), s64)
    for tag, weights, pres in (("", None, present), ("_w", pw, None)):
        L64, g64 = po.contrast(feat, proto, labels, T, pres, weights, eps=eps)
        L32, g32 = po.contrast(feat, proto, labels, T, pres, weights, eps=eps, dtype=torch.float32)
        r.update({"L64" + tag: L64, "g64" + tag: g64, "yard_L" + tag: abs(L32.double().item() - L64.item()), "yard_g" + tag: yard(g32, g64)})
    return r


def ratio(e, b):
    return e / b if b > 0 else (0.0 if e == 0 else float("inf"))


@pytest.mark.parametrize("i", range(len(PARAMS)))
def test_prototypes_similarity_loss_and_gradient_against_float64(dev, i):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    r = reference(i)
    K, S1, T = r["K"], r["per_image"], r["T"]
    f, lab, pw = r["feat"].to(dev), r["labels"].to(dev), r["pw"].to(dev)
    keep = (f.clone(), lab.clone(), pw.clone())
    worst = {}

    def check(what, got, want, yardstick):
        e, b = maxerr(got, want), bound(yardstick, want)
        print(f"{name_of(i)}: {what} error {e:.3e} / bound {b:.3e} (yardstick {yardstick:.3e})")
        worst[what.split()[0]] = max(worst.get(what.split()[0], 0.0), ratio(e, b))
        assert e <= b, (what, e, b)

    # pooling: plain, weighted, unnormalised; the mass against an integer count; a zero-mass prototype exactly 0
    proto, mass = ops.class_prototypes(f, lab, K, per_image=S1)
    assert proto.dtype == mass.dtype == torch.float32 and tuple(proto.shape) == tuple(r["p64"].shape) and tuple(mass.shape) == tuple(r["m64"].shape)
    check("prototypes", proto, r["p64"], r["yard_p"])
    assert torch.equal(mass.cpu().double(), r["m64"]) and torch.equal(r["m64"], r["m64"].round())
    assert torch.equal((proto != 0).any(dim=2).cpu() | (r["m64"] > 0), r["m64"] > 0)
    pw_proto, pw_mass = ops.class_prototypes(f, lab, K, pixel_weight=pw, per_image=S1)
    check("prototypes weighted", pw_proto, r["p64_w"], r["yard_p_w"])
    check("mass weighted", pw_mass, r["m64_w"], r["yard_m_w"])
    assert not pw_proto[(pw_mass == 0)].any()
    check("prototypes raw", ops.class_prototypes(f, lab, K, per_image=S1, normalize=False)[0], r["raw64"], r["yard_raw"])

    # similarity on the oracle's prototypes: every activation, present given and None
    q, present = r["proto"].to(dev), r["present"].to(dev)
    for act in ("none", "relu", "softmax"):
        s = ops.prototype_similarity(f, q, activation=act, temperature=T, present=present)
        check(f"similarity {act}", s, r["s64_" + act], r["yard_s_" + act])
        if act == "softmax":
            rows = s.cpu().double().sum(dim=1)
            has = r["present"].any(dim=1)
            has = (has if S1 else has.expand(f.shape[0]))[:, None, None].expand_as(rows)
            if has.any():                                                   # rows sum to 1 (to 0 where no class is present)
                assert (rows[has] - 1).abs().max().item() <= bound(r["yard_s_softmax"], torch.ones(1))
            assert not rows[~has].any()
            assert not s.cpu()[~(r["present"] if S1 else r["present"].expand(f.shape[0], K))].any()          # an absent class: exactly 0
        else:
            assert torch.equal(s, ops.prototype_similarity(f, q, activation=act, temperature=T))                 # present plays no part
    assert torch.equal(ops.prototype_similarity(f, q, activation="relu"), ops.prototype_similarity(f, q).clamp_min(0))

    # the loss and its gradient, plain with present and weighted without; forward only gives the same bits
    for tag, kw in (("", dict(present=present)), ("_w", dict(pixel_weight=pw))):
        fg = f.clone().requires_grad_()
        L = ops.prototype_contrast_loss(fg, q, lab, temperature=T, **kw)
        L.backward()
        assert L.dtype == torch.float32 and L.dim() == 0 and tuple(fg.grad.shape) == tuple(f.shape)
        check("loss" + tag, L, r["L64" + tag], r["yard_L" + tag])
        check("gradient" + tag, fg.grad, r["g64" + tag], r["yard_g" + tag])
        assert torch.equal(L, ops.prototype_contrast_loss(f, q, lab, temperature=T, **kw))
        uncounted = (r["g64" + tag] == 0).all(dim=1)
        assert not fg.grad.cpu()[uncounted[:, None].expand_as(fg.grad)].any()
    assert all(torch.equal(a, b) for a, b in zip(keep, (f, lab, pw)))                # inputs untouched
    report_line(f"prototype {name_of(i)}: device error / bound: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("i", (4, 7, 12))
def test_absent_class_and_everything_ignored(dev, i):
    from weaklysuperviseddl_amd import ops
    for variant in ("absent", "ignored"):
        r = reference(i, variant)
        f, lab, K = r["feat"].to(dev).requires_grad_(), r["labels"].to(dev), r["K"]
        proto, mass = ops.class_prototypes(f, lab, K, per_image=r["per_image"])
        assert torch.equal(mass.cpu().double(), r["m64"])
        assert maxerr(proto, r["p64"]) <= bound(r["yard_p"], r["p64"])
        L = ops.prototype_contrast_loss(f, r["proto"].to(dev), lab, temperature=r["T"], present=mass > 0)
        L.backward()
        if variant == "ignored":
            assert not mass.any() and not proto.any() and L.item() == 0.0 and not f.grad.any()
            sm = ops.prototype_similarity(f, proto, activation="softmax", present=mass > 0)
            assert not sm.any() and not ops.prototype_similarity(f, proto).any()
        else:
            if r["per_image"]:
                assert mass[0, K - 1].item() == 0 and not proto[0, K - 1].any()
            assert abs(L.item() - r["L64"].item()) <= bound(r["yard_L"], r["L64"])
            assert maxerr(f.grad, r["g64"]) <= bound(r["yard_g"], r["g64"])


def test_pooling_on_a_map_of_more_than_1024_tiles(dev):
    """The norm pass takes 64-pixel tiles from 1024 tiles on (16-pixel tiles below): 1 x 3 x 256 x 257, beyond the shapes above."""
    from weaklysuperviseddl_amd import ops
    feat, labels = po.make_features(1, 3, 256, 257, 70), po.make_labels(1, 256, 257, 3, 71)
    p64, m64 = po.prototypes(feat, labels, 3)
    p32, _ = po.prototypes(feat, labels, 3, dtype=torch.float32)
    proto, mass = ops.class_prototypes(feat.to(dev), labels.to(dev), 3)
    assert torch.equal(mass.cpu().double(), m64) and maxerr(proto, p64) <= bound(yard(p32, p64), p64)
    s64 = po.similarity(feat, p64.float(), "softmax", 0.1)
    s = ops.prototype_similarity(feat.to(dev), p64.float().to(dev), activation="softmax", temperature=0.1)
    assert maxerr(s, s64) <= bound(yard(po.similarity(feat, p64.float(), "softmax", 0.1, dtype=torch.float32), s64), s64)


def test_zero_vectors_the_clamped_norm_and_out_of_range_labels(dev):
    """An exactly-zero feature vector, ignored and counted, with the default eps (similarity 0, gradient v / eps) and the eps =
    1e-3 branch on a short non-zero vector; NaN for an out-of-range label at that pixel only under 'none'."""
    from weaklysuperviseddl_amd import ops
    B, D, h, w, K = 2, 5, 5, 7, 3
    feat = po.make_features(B, D, h, w, 50)
    feat[0, :, 0, 0] = 0.0
    feat[0, :, 0, 1] = 0.0
    feat[1, :, 2, 3] *= 1e-4
    labels = po.make_labels(B, h, w, K, 51)
    labels[0, 0, 0], labels[0, 0, 1], labels[1, 2, 3] = 1, po.IGNORE, 2
    f, lab = feat.to(dev), labels.to(dev)
    for eps in (1e-12, 1e-3):
        p64, m64 = po.prototypes(feat, labels, K, eps=eps)
        p32, _ = po.prototypes(feat, labels, K, eps=eps, dtype=torch.float32)
        proto, mass = ops.class_prototypes(f, lab, K, eps=eps)
        assert maxerr(proto, p64) <= bound(yard(p32, p64), p64) and torch.equal(mass.cpu().double(), m64)
        q = p64.float()
        s64 = po.similarity(feat, q, eps=eps)
        s = ops.prototype_similarity(f, q.to(dev), eps=eps)
        assert maxerr(s, s64) <= bound(yard(po.similarity(feat, q, eps=eps, dtype=torch.float32), s64), s64)
        assert not s[0, :, 0, :2].any()
        for reduction in ("mean", "sum", "none"):
            L64, g64 = po.contrast(feat, q, labels, 0.1, reduction=reduction, eps=eps)
            L32, g32 = po.contrast(feat, q, labels, 0.1, reduction=reduction, eps=eps, dtype=torch.float32)
            fg = f.clone().requires_grad_()
            L = ops.prototype_contrast_loss(fg, q.to(dev), lab, reduction=reduction, eps=eps)
            L.sum().backward()
            assert maxerr(L, L64) <= bound(yard(L32, L64), L64), (eps, reduction)
            assert maxerr(fg.grad, g64) <= bound(yard(g32, g64), g64), (eps, reduction)
            assert not fg.grad[0, :, 0, 1].any() and fg.grad[0, :, 0, 0].abs().max().item() > 0
            if reduction == "none":
                assert tuple(L.shape) == (B, h, w) and L[0, 0, 1].item() == 0.0
    bad = labels.clone()
    bad[1, 4, 6] = K
    fg = f.clone().requires_grad_()
    L = ops.prototype_contrast_loss(fg, q.to(dev), bad.to(dev), reduction="none")
    L.sum().backward()
    assert torch.isnan(L[1, 4, 6]) and torch.isnan(L).sum().item() == 1
    assert torch.isnan(fg.grad[1, :, 4, 6]).all() and torch.isnan(fg.grad).sum().item() == D
    assert torch.isnan(ops.prototype_contrast_loss(f, q.to(dev), bad.to(dev)))
    assert torch.equal(ops.class_prototypes(f, bad.to(dev), K)[1].cpu().double(), po.prototypes(feat, bad, K)[1])      # not pooled


def test_call_mechanics(dev):
    """Second calls bit-identical, out= reuse, detached results, a bool and a uint8 present mask alike."""
    from weaklysuperviseddl_amd import ops
    r = reference(7)
    f, lab, pw, K = r["feat"].to(dev), r["labels"].to(dev), r["pw"].to(dev), r["K"]
    a, b = ops.class_prototypes(f, lab, K, pixel_weight=pw), ops.class_prototypes(f, lab, K, pixel_weight=pw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not a[0].requires_grad
    out = (torch.full_like(a[0], 7.0), torch.full_like(a[1], 7.0))
    got = ops.class_prototypes(f.requires_grad_(), lab, K, pixel_weight=pw, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], a[0]) and torch.equal(out[1], a[1]) and got[0].grad_fn is None
    f = f.detach()
    present = a[1] > 0
    s1 = ops.prototype_similarity(f, a[0], activation="softmax", temperature=0.1, present=present)
    so = torch.full_like(s1, 7.0)
    assert ops.prototype_similarity(f, a[0], activation="softmax", temperature=0.1, present=present.to(torch.uint8), out=so) is so
    assert torch.equal(s1, so) and torch.equal(s1, ops.prototype_similarity(f, a[0], activation="softmax", temperature=0.1, present=present))
    grads = []
    for _ in range(2):
        fg = f.clone().requires_grad_()
        L = ops.prototype_contrast_loss(fg, a[0], lab, present=present, pixel_weight=pw)
        L.backward()
        grads.append((L.clone(), fg.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    fg = f.clone().requires_grad_()
    (3.0 * ops.prototype_contrast_loss(fg, a[0], lab, present=present, pixel_weight=pw)).backward()
    assert torch.allclose(fg.grad, 3.0 * grads[0][1], rtol=1e-6, atol=0)
    with pytest.raises(ops.WsdlError):
        ops.prototype_similarity(f, a[0], out=f[:, :K])
    with pytest.raises(ops.WsdlError):
        ops.class_prototypes(f, lab, K, per_image=False, out=out)


def test_strided_features_that_need_a_gradient(dev):
    """Non-contiguous features: the ops work on a dense copy, the gradient still reaches the argument."""
    from weaklysuperviseddl_amd import ops
    r = reference(4)
    f, lab, q = r["feat"].to(dev), r["labels"].to(dev), r["proto"].to(dev)
    base = torch.cat([f, f], dim=1).requires_grad_()
    view = base[:, 1:1 + f.shape[1]]
    assert not view.is_contiguous()
    ops.prototype_contrast_loss(view, q, lab).backward()
    ref = view.detach().contiguous().requires_grad_()
    ops.prototype_contrast_loss(ref, q, lab).backward()
    assert torch.equal(base.grad[:, 1:1 + f.shape[1]], ref.grad) and not base.grad[:, 0].any() and ref.grad.abs().max().item() > 0
    assert torch.equal(ops.class_prototypes(view, lab, r["K"])[0], ops.class_prototypes(ref.detach(), lab, r["K"])[0])
    assert torch.equal(ops.prototype_similarity(view, q), ops.prototype_similarity(ref.detach(), q))


@pytest.mark.parametrize("i", (5, 9, 14))
def test_autograd_of_a_torch_composition_equals_the_fused_gradient(dev, i):
    """F.normalize + einsum + cross entropy under torch autograd ON THE DEVICE in float32 against the fused gradient.  The
    composition is one more float32 evaluation of the same contract, so it is held to the standing bound itself: at most ``b =
    max(4 x yardstick, 2^-23 |value|)`` from float64, the yardstick being the CPU float32 oracle's error, as for the fused kernel.
    Two results within ``b`` of float64 are within ``2 b`` of each other: that is the bound of fused against composition (no
    measured error of either side enters it).  (Absent classes get the logit -1e30 in the composition: ``exp`` underflows to an
    exact 0, as for a class that is left out.)"""
    import torch.nn.functional as F
    from weaklysuperviseddl_amd import ops
    r = reference(i)
    f, lab, q, T = r["feat"].to(dev), r["labels"].to(dev), r["proto"].to(dev), r["T"]
    present = r["present"].to(dev)
    fg = f.clone().requires_grad_()
    ops.prototype_contrast_loss(fg, q, lab, temperature=T, present=present).backward()
    ft = f.clone().requires_grad_()
    qn = F.normalize(q, dim=2)
    qn = qn.expand(f.shape[0], -1, -1) if qn.shape[0] == 1 else qn
    z = torch.einsum("bdhw,bkd->bkhw", F.normalize(ft, dim=1), qn) / T
    on = (present.expand(f.shape[0], -1) if present.shape[0] == 1 else present)[:, :, None, None]
    z = torch.where(on, z, torch.full_like(z, -1e30))
    y = torch.where((lab != po.IGNORE) & torch.gather(on[:, :, 0, 0], 1, lab.clamp(0, r["K"] - 1).flatten(1)).view_as(lab), lab,
                    torch.full_like(lab, -100))
    F.cross_entropy(z, y, ignore_index=-100).backward()
    b = bound(r["yard_g"], r["g64"])
    e_fused, e_torch, e_both = maxerr(fg.grad, r["g64"]), maxerr(ft.grad, r["g64"]), maxerr(fg.grad, ft.grad.cpu().double())
    print(f"{name_of(i)}: fused {e_fused:.3e}, torch composition {e_torch:.3e}, fused against composition {e_both:.3e}, bound {b:.3e}")
    assert e_fused <= b, (e_fused, b)
    assert e_torch <= b, (e_torch, b)
    assert e_both <= 2 * b, (e_both, b)


@pytest.mark.parametrize("momentum", (0.0, 0.99, 1.0))
def test_prototype_ema_against_the_oracle(dev, momentum):
    from weaklysuperviseddl_amd import ops
    K, D = 5, 70
    g = torch.Generator().manual_seed(60)
    p1, p2 = torch.randn(1, K, D, generator=g), torch.randn(1, K, D, generator=g)
    m1, m2 = torch.tensor([[3.0, 0.0, 1.0, 0.0, 2.0]]), torch.tensor([[1.0, 0.0, 0.0, 4.0, 0.5]])
    bank, count = torch.zeros(K, D, device=dev), torch.zeros(K, dtype=torch.int64, device=dev)
    b64, c64 = bank.cpu().double(), count.cpu()
    for p, m in ((p1, m1), (p2, m2), (p1, m2)):
        assert ops.prototype_ema_(bank, count, p.to(dev), m.to(dev), momentum) is bank
        old = b64
        b64, c64 = po.ema(b64.float(), c64, p, m, momentum)            # (each step from the float bank the device holds)
        assert count.tolist() == c64.tolist()
        assert maxerr(bank, b64) <= ULP * b64.abs().max().item()
        assert torch.equal(bank.cpu()[m[0] == 0].double(), old[m[0] == 0])         # a class of zero mass is untouched
        b64 = bank.cpu().double()
    assert count.tolist() == [3, 0, 1, 2, 3] and not bank[1].any()
    first = torch.zeros(K, D, device=dev)
    ops.prototype_ema_(first, torch.zeros(K, dtype=torch.int64, device=dev), p1[0].to(dev), m1[0].to(dev), momentum)   # (K,D) / (K,) forms
    assert torch.equal(first.cpu()[m1[0] > 0], p1[0][m1[0] > 0]) and not first.cpu()[m1[0] == 0].any()       # the first touch takes proto as it is
    if momentum == 1.0:
        keep = bank.clone()
        ops.prototype_ema_(bank, count, p2.to(dev), torch.ones(1, K, device=dev), 1.0)
        assert torch.equal(bank[[0, 2, 3, 4]], keep[[0, 2, 3, 4]]) and torch.equal(bank[1].cpu(), p2[0, 1])


@pytest.mark.parametrize("source", ("batch", "image", "bank"))
def test_module_is_the_composition_of_the_ops(dev, source):
    from weaklysuperviseddl_amd import ops, nn as wnn
    r = reference(5)
    K, lab = r["K"], r["labels"].to(dev)
    crit = wnn.PrototypeContrastLoss(K, 0.07, source, momentum=0.9)
    bank, count = torch.zeros(K, r["feat"].shape[1], device=dev), torch.zeros(K, dtype=torch.int64, device=dev)
    for step in range(2):                                                               # two bank updates
        f = (r["feat"] * (1.0 + step)).roll(step, dims=1).to(dev)
        f1, f2 = f.clone().requires_grad_(), f.clone().requires_grad_()
        L1 = crit(f1, lab)
        proto, mass = ops.class_prototypes(f2.detach(), lab, K, per_image=source == "image")
        if source == "bank":
            ops.prototype_ema_(bank, count, proto, mass, 0.9)
            proto, present = bank[None], count[None] > 0
            assert torch.equal(crit.bank, bank) and torch.equal(crit.count, count) and count.max().item() == step + 1
        else:
            present = mass > 0
        L2 = ops.prototype_contrast_loss(f2, proto, lab, temperature=0.07, present=present)
        L1.backward()
        L2.backward()
        assert torch.equal(L1, L2) and torch.equal(f1.grad, f2.grad) and L1.item() > 0 and f1.grad.abs().max().item() > 0
    assert sorted(crit.state_dict()) == (["bank", "count"] if source == "bank" else [])     # the bank is checkpointed, scratch is not
    if source == "bank":
        twin = wnn.PrototypeContrastLoss(K, 0.07, source, momentum=0.9)
        twin.load_state_dict(crit.state_dict())
        assert torch.equal(twin.bank, bank) and torch.equal(twin.count, count) and twin.bank.device == bank.device
        assert torch.equal(twin(f.detach(), lab), crit(f.detach(), lab))                     # the same third update from the same bank
        crit.reset()
        assert not crit.bank.any() and not crit.count.any()
    assert not isinstance(crit, wnn._Criterion)


def test_launch_plans_replay_loss_and_similarity(dev):
    from weaklysuperviseddl_amd import ops, plan
    r = reference(7)
    f, lab, q, K = r["feat"].to(dev).requires_grad_(), r["labels"].to(dev), r["proto"].to(dev), r["K"]

    def step():
        L = ops.prototype_contrast_loss(f, q, lab, temperature=0.1)
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

    fd = f.detach()
    outs = (torch.empty(fd.shape[0], K, fd.shape[1], device=dev), torch.empty(fd.shape[0], K, device=dev))
    sim = torch.empty(fd.shape[0], K, *fd.shape[2:], device=dev)

    def pool_and_compare():
        proto, _ = ops.class_prototypes(fd, lab, K, out=outs)
        return ops.prototype_similarity(fd, proto, activation="softmax", temperature=0.1, out=sim)
    p2, res = plan.record(pool_and_compare)
    assert res is sim and p2.stats["kernels"] == 5 and torch.equal(sim, pool_and_compare().clone())
    first = sim.clone()
    fd.copy_((fd * 0.7 + 0.1 * fd.flip(-2)).contiguous())
    lab.copy_(lab.flip(-2).contiguous())
    p2.replay()
    torch.cuda.synchronize()
    replayed = sim.clone()
    assert torch.equal(replayed, pool_and_compare()) and not torch.equal(replayed, first)


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


def test_projection_net_prototype_cam_and_generate_pseudo_masks(dev):
    """A 64 x 64 image through ProjectionNet: finite embeddings of the documented shape, finite non-zero gradients on the four
    head convolutions only.  prototype_cam and generate_prototype_pseudo_masks equal the composition of the ops bit for bit; an
    image without a foreground seed keeps its CAM; prototype None is generate_pseudo_masks."""
    from weaklysuperviseddl_amd import ops, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import (ProjectionNet, TrunkFeatures, affinity_labels_from_cam, generate_pseudo_masks,
                                                         generate_prototype_pseudo_masks)
    from weaklysuperviseddl_amd.TraditionalModel.PsuedoMasks import nearest_resize_index, prototype_cam, seeds_from_cam
    model, gen = _cam_generator(dev)
    torch.manual_seed(1)
    net = ProjectionNet(model, dim=32).to(dev).train()
    assert not net.trunk.training
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    feat = net(x)
    assert tuple(feat.shape) == (2, 32, 8, 8) and torch.isfinite(feat).all()
    cam = torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    labels = affinity_labels_from_cam(cam, 0.3, 0.6, feat.shape[-2:])
    wnn.PrototypeContrastLoss(2)(feat, labels).backward()
    with_grad = sorted(k for k, p in net.named_parameters() if p.grad is not None)
    assert with_grad == ["f8_3.weight", "f8_4.weight", "f8_5.weight", "proj.weight"]
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, k

    tf = TrunkFeatures(model, "layer4").to(dev)
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 224, 224, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_prototype_pseudo_masks(loader, gen, None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    generate_prototype_pseudo_masks(loader, gen, dict(net=tf, lo=0.1, hi=0.4, temperature=0.2), **kw)
    got = torch.stack(generate_pseudo_masks.last_masks)
    imgs = loader[0][0].to(dev)
    cam, _ = gen.generate_batch(imgs, alpha=1.0, class_idx=loader[0][1][0].to(dev), thresh=0.3)
    ft = tf(imgs)
    assert tuple(ft.shape) == (2, 2048, 14, 14) and not ft.requires_grad
    seeds = seeds_from_cam(cam, 0.1, 0.4)
    small = seeds[:, nearest_resize_index(14, 224, dev)][:, :, nearest_resize_index(14, 224, dev)].contiguous()
    proto, mass = ops.class_prototypes(ft, small, 2)
    sim = ops.prototype_similarity(ft, proto, activation="softmax", temperature=0.2)
    back = ops.bilinear_resize(sim[:, 1:2].contiguous(), (224, 224))[:, 0]
    both = (mass > 0).all(dim=1)
    pc = prototype_cam(imgs, cam, tf, lo=0.1, hi=0.4, temperature=0.2)
    assert torch.equal(pc, torch.where(both[:, None, None], back, cam))
    assert torch.equal(got, ops.keep_largest_batched((pc >= 0.3).to(torch.uint8))) and got.dtype == torch.uint8
    assert both.any().item(), "the fixture should have both kinds of seed in some image"
    flat = cam.clone()
    flat[1] = 0.01                                                                      # no foreground seed: the CAM is kept exactly
    kept = prototype_cam(imgs, flat, tf, lo=0.1, hi=0.4, temperature=0.2)
    assert torch.equal(kept[1], flat[1]) and torch.equal(kept[0], pc[0])


def test_train_projection_net_takes_steps(dev):
    """Two batches of 64 x 64 images, one epoch: a finite loss, the four head convolutions move, the trunk does not."""
    from weaklysuperviseddl_amd.TraditionalModel import ProjectionNet, train_projection_net
    model, _ = _cam_generator(dev)
    torch.manual_seed(2)
    net = ProjectionNet(model, dim=16)
    before = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
    g = torch.Generator().manual_seed(8)
    loader = [(torch.rand(2, 3, 64, 64, generator=g), None) for _ in range(2)]
    ramp = torch.linspace(0, 1, 64).view(1, 1, 64).expand(2, 64, 64).contiguous()
    history = train_projection_net(net, loader, [ramp, ramp.transpose(1, 2).contiguous()], lo=0.3, hi=0.6, source="bank", device=dev, log=None)
    assert len(history) == 1 and history[0] == history[0] and 0 < history[0] < float("inf") and not net.training
    for k, p in net.named_parameters():
        same = torch.equal(p.detach().cpu(), before[k])
        assert same == k.startswith("trunk."), k
