"""CPU-side checks of the prototype ops: the float64 oracle (tests/prototype_oracle.py) against independent formulations -
F.normalize + einsum + F.cross_entropy under torch autograd, explicit per-pixel loops, central differences - and the host-side
validation (check_prototype_options, the modules, generate_prototype_pseudo_masks, ProjectionNet).  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prototype_oracle as po  # noqa: E402


def torch_formulation(feat, proto, labels, temperature, classes, pixel_weight, eps, reduction="mean"):
    """The contract in tensor-library ops, float64, gradient by autograd.  ``classes``: the indices of the present classes (one
    segment) - absent ones are left out of the logits and their pixels are ignored."""
    f = feat.double().requires_grad_()
    q = F.normalize(proto.double()[0], dim=1, eps=eps)[classes]
    z = torch.einsum("bdhw,kd->bkhw", F.normalize(f, dim=1, eps=eps), q) / temperature
    remap = torch.full((256,), -100, dtype=torch.int64)
    remap[torch.as_tensor(classes)] = torch.arange(len(classes))
    y = remap[labels]
    l = F.cross_entropy(z, y, ignore_index=-100, reduction="none")
    w = torch.ones_like(l) if pixel_weight is None else pixel_weight.double()
    total = (w * (y >= 0)).sum()
    loss = (l * w).sum() / total if reduction == "mean" else (l * w).sum() if reduction == "sum" else l * w
    (loss.sum()).backward()
    return loss.detach(), f.grad, z.detach()


@pytest.mark.parametrize("eps", (1e-12, 1e-3))
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_oracle_equals_normalize_einsum_cross_entropy_autograd(eps, reduction):
    B, D, h, w, K = 2, 6, 5, 7, 4
    feat = po.make_features(B, D, h, w, 1)
    feat[0, :, 0, 0] = 0.0                                  # an exactly-zero vector, counted
    feat[1, :, 2, 3] *= 1e-4                                # below eps = 1e-3: the clamped branch with a non-zero vector
    labels = po.make_labels(B, h, w, K, 2)
    labels[0, 0, 0] = 1
    labels[1, 2, 3] = 2
    pw = po.make_weights(B, h, w, 3)
    pw[0, 0, 0] = pw[1, 2, 3] = 1.5
    proto, _ = po.prototypes(feat, labels, K, per_image=False)
    for classes, weights in (([0, 1, 2, 3], None), ([0, 2, 3], pw), ([1, 2], pw)):
        present = torch.zeros(1, K, dtype=torch.bool)
        present[0, classes] = True
        L, g = po.contrast(feat, proto, labels, 0.1, present, weights, reduction=reduction, eps=eps)
        L2, g2, z = torch_formulation(feat, proto, labels, 0.1, classes, weights, eps, reduction)
        assert torch.allclose(L, L2, rtol=1e-12, atol=1e-13), (classes, L, L2)
        assert torch.allclose(g, g2, rtol=1e-9, atol=1e-9 * g2.abs().max().item()), (classes, (g - g2).abs().max())
        sim = po.similarity(feat, proto, "none", eps=eps)[:, classes]
        assert torch.allclose(sim, z * 0.1, rtol=1e-12, atol=1e-14)
        soft = po.similarity(feat, proto, "softmax", 0.1, present, eps=eps)
        assert torch.allclose(soft[:, classes], z.softmax(dim=1), rtol=1e-12, atol=1e-15)
        absent = [k for k in range(K) if k not in classes]
        assert not soft[:, absent].any() and torch.allclose(soft.sum(dim=1), torch.ones(B, h, w, dtype=torch.float64))
        assert torch.equal(po.similarity(feat, proto, "relu", eps=eps), po.similarity(feat, proto, "none", eps=eps).clamp_min(0))
        ignored = (labels == po.IGNORE) | ~present[0][labels.clamp(0, K - 1)]
        assert not g[ignored[:, None].expand_as(g)].any()                   # an uncounted pixel gets exact zeros
    if eps == 1e-3:
        assert g[1, :, 2, 3].abs().max() > 0 and g[0, :, 0, 0].abs().max() > 0      # the clamped branch is not a zero gradient


def test_oracle_per_image_prototypes_and_float32():
    B, D, h, w, K = 3, 5, 4, 6, 3
    feat, labels = po.make_features(B, D, h, w, 4), po.make_labels(B, h, w, K, 5, "absent")
    proto, mass = po.prototypes(feat, labels, K)
    assert mass[0, K - 1] == 0 and not proto[0, K - 1].any()
    L, g = po.contrast(feat, proto, labels, 0.07, mass > 0)
    want = 0.0
    for b in range(B):                                      # image by image against the one-segment formulation
        classes = [k for k in range(K) if mass[b, k] > 0]
        Lb, gb, _ = torch_formulation(feat[b:b + 1], proto[b:b + 1], labels[b:b + 1], 0.07, classes, None, 1e-12, "sum")
        want = want + Lb
        n = ((labels != po.IGNORE) & (labels < K)).sum()
        assert torch.allclose(g[b:b + 1] * n, gb, rtol=1e-9, atol=1e-12)
    assert torch.allclose(L * n, want, rtol=1e-12)
    L32, g32 = po.contrast(feat, proto, labels, 0.07, mass > 0, dtype=torch.float32)
    p32, m32 = po.prototypes(feat, labels, K, dtype=torch.float32)
    assert L32.dtype == g32.dtype == p32.dtype == m32.dtype == torch.float32
    assert abs(L32.item() - L.item()) < 1e-5 and (g32.double() - g).abs().max() < 1e-6 and (p32.double() - proto).abs().max() < 1e-6


@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("per_image", (True, False))
def test_oracle_prototypes_equal_a_per_pixel_loop(per_image, normalize):
    B, D, h, w, K = 2, 3, 4, 5, 3
    feat, labels, pw = po.make_features(B, D, h, w, 6), po.make_labels(B, h, w, K, 7), po.make_weights(B, h, w, 8)
    labels[0, 0, 0], labels[1, 1, 1] = 7, -1                # outside [0, K): not pooled
    for weights in (None, pw):
        proto, mass = po.prototypes(feat, labels, K, weights, per_image, normalize)
        S = B if per_image else 1
        num, den = torch.zeros(S, K, D, dtype=torch.float64), torch.zeros(S, K, dtype=torch.float64)
        for b in range(B):
            for y in range(h):
                for x in range(w):
                    k = int(labels[b, y, x])
                    if k == po.IGNORE or not 0 <= k < K:
                        continue
                    v = feat[b, :, y, x].double()
                    if normalize:
                        v = v / max(float(v.pow(2).sum().sqrt()), 1e-12)
                    wt = 1.0 if weights is None else float(weights[b, y, x])
                    num[b if per_image else 0, k] += wt * v
                    den[b if per_image else 0, k] += wt
        assert torch.allclose(mass, den, rtol=1e-13, atol=0)
        assert torch.allclose(proto, num / den[..., None], rtol=1e-12, atol=1e-15)
        if weights is None:
            assert torch.equal(mass, mass.round())


def test_oracle_gradient_against_central_differences():
    feat = po.make_features(1, 3, 2, 2, 9)
    labels = torch.tensor([[[0, 1], [1, po.IGNORE]]])
    proto = po.make_features(1, 2, 3, 1, 10)[..., 0].double()          # (1, 2, 3): constants
    pw = torch.tensor([[[1.0, 0.5], [2.0, 1.0]]])
    for reduction in ("mean", "sum"):
        _, g = po.contrast(feat, proto, labels, 0.5, None, pw, reduction=reduction)
        num = torch.zeros_like(g)
        f64, step = feat.double(), 1e-6
        for i in range(f64.numel()):
            e = torch.zeros(f64.numel(), dtype=torch.float64)
            e[i] = step
            e = e.view_as(f64)
            num.view(-1)[i] = (po.contrast(f64 + e, proto, labels, 0.5, None, pw, reduction=reduction)[0] -
                               po.contrast(f64 - e, proto, labels, 0.5, None, pw, reduction=reduction)[0]) / (2 * step)
        assert torch.allclose(g, num, rtol=1e-6, atol=1e-8), (g - num).abs().max()
        assert not g[0, :, 1, 1].any()


def test_oracle_special_cases():
    feat, K = po.make_features(2, 4, 3, 3, 11), 3
    ignored = po.make_labels(2, 3, 3, K, 12, "ignored")
    proto, mass = po.prototypes(feat, ignored, K)
    assert not proto.any() and not mass.any()
    L, g = po.contrast(feat, proto, ignored, 0.1, mass > 0)
    assert L.item() == 0.0 and not g.any()
    labels = po.make_labels(2, 3, 3, K, 13)
    labels[1, 2, 2] = 9                                                 # out of range: NaN at that pixel only under 'none'
    proto, mass = po.prototypes(feat, labels, K, per_image=False)
    L, g = po.contrast(feat, proto, labels, 0.1, reduction="none")
    assert torch.isnan(L[1, 2, 2]) and torch.isnan(L).sum() == 1 and torch.isnan(g[1, :, 2, 2]).all() and torch.isnan(g).sum() == 4
    assert torch.isnan(po.contrast(feat, proto, labels, 0.1)[0])
    assert not po.similarity(feat, torch.zeros(1, K, 4))[:, 0].any()    # a zero prototype gives 0
    bank, count = torch.zeros(K, 4), torch.zeros(K, dtype=torch.int64)
    mass = torch.tensor([[2.0, 0.0, 1.0]])
    b1, c1 = po.ema(bank, count, proto, mass, 0.9)
    assert torch.equal(b1[0], proto[0, 0]) and not b1[1].any() and c1.tolist() == [1, 0, 1]
    b2, c2 = po.ema(b1, c1, proto * 2, mass, 0.9)
    assert torch.allclose(b2[0], 1.1 * proto[0, 0]) and c2.tolist() == [2, 0, 2]


def test_check_prototype_options_refusals():
    from weaklysuperviseddl_amd import ops
    f, lab = torch.zeros(2, 4, 6, 6), torch.zeros(2, 6, 6, dtype=torch.int64)
    proto, mass, present = torch.zeros(2, 3, 4), torch.zeros(2, 3), torch.ones(2, 3, dtype=torch.bool)
    bank, count = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64)
    bad = [
        dict(feat=f[0]), dict(feat=f.double()), dict(feat=f, labels=lab.int()), dict(feat=f, labels=lab[:, :5]), dict(feat=f, labels=lab[0]),
        dict(feat=f, pixel_weight=lab), dict(feat=f, pixel_weight=torch.zeros(2, 6, 5)), dict(feat=torch.zeros(2, 0, 6, 6)),
        dict(feat=torch.zeros(1, 2049, 1, 1)), dict(feat=torch.zeros(1, 1, 1024, 1025)),
        dict(num_classes=0), dict(num_classes=33), dict(num_classes=2.0), dict(num_classes=True),
        dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(temperature="1"),
        dict(eps=0.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=float("nan")),
        dict(activation="sigmoid"), dict(reduction="max"),
        dict(feat=f, proto=torch.zeros(3, 3, 4)), dict(feat=f, proto=torch.zeros(2, 3, 5)), dict(feat=f, proto=torch.zeros(2, 33, 4)),
        dict(feat=f, proto=proto[0]), dict(feat=f, proto=proto, num_classes=4), dict(feat=f, proto=proto.double()),
        dict(feat=f, proto=proto, present=present[:1]), dict(feat=f, proto=proto, present=torch.ones(2, 4, dtype=torch.bool)),
        dict(feat=f, proto=proto, present=present.float()), dict(feat=f, proto=proto, mass=mass[:1]), dict(proto=proto, mass=torch.zeros(2, 4)),
        dict(proto=proto, mass=mass, bank=bank, count=count),               # the bank takes one segment
        dict(proto=proto[:1], mass=mass[:1], bank=torch.zeros(3, 5), count=count), dict(proto=proto[:1], mass=mass[:1], bank=bank, count=count[:2]),
        dict(proto=proto[:1], mass=mass[:1], bank=bank, count=count.int()), dict(proto=proto[:1], mass=mass[:1], bank=proto[0], count=count),
        dict(out=torch.zeros(2, 3, 6, 6)), dict(feat=f, proto=proto, out=torch.zeros(2, 3, 6, 5)), dict(feat=f, proto=proto, out=torch.zeros(2, 3, 6, 6).double()),
        dict(feat=f, proto=proto, out=torch.zeros(2, 3, 6, 12)[..., ::2]), dict(feat=f, proto=proto, out=torch.zeros(2, 3, 6, 6, requires_grad=True)),
        dict(feat=f, proto=f.view(-1)[:24].view(2, 3, 4), out=f.view(-1)[:216].view(2, 3, 6, 6)),
        dict(feat=f, num_classes=3, out=torch.zeros(2, 3, 4)), dict(feat=f, num_classes=3, out=(torch.zeros(2, 3, 5), torch.zeros(2, 3))),
        dict(feat=f, num_classes=3, out=(torch.zeros(2, 3, 4), torch.zeros(1, 3))), dict(feat=f, num_classes=3, out=(f.view(-1)[:24].view(2, 3, 4), torch.zeros(2, 3))),
    ]
    for kw in bad:
        with pytest.raises(ops.WsdlError):
            ops.check_prototype_options(**kw)
    # the place comes last: everything else about these is right, so a host tensor is what is refused
    for kw in (dict(feat=f, labels=lab, num_classes=3), dict(feat=f, proto=proto, present=present), dict(proto=proto[:1], mass=mass[:1], bank=bank, count=count)):
        with pytest.raises(ops.WsdlError, match="device tensor"):
            ops.check_prototype_options(**kw)
    for fn in (lambda: ops.class_prototypes(f, lab, 3), lambda: ops.prototype_similarity(f, proto), lambda: ops.prototype_contrast_loss(f, proto, lab),
               lambda: ops.prototype_ema_(bank, count, proto[:1], mass[:1], 0.9), lambda: ops.prototype_ema_(bank, None, proto[0], mass[0], 0.9)):
        with pytest.raises(ops.WsdlError):
            fn()
    assert ops.check_prototype_options(num_classes=32, temperature=0.07, eps=1e-12, momentum=1, activation="relu", reduction="none") == (32, None)
    assert ops.prototype_workspace(2, 448, 21, 32, 32) > 0 and ops.prototype_workspace(1, 2049, 2, 4, 4) == 0
    assert ops.prototype_workspace(1, 4, 33, 4, 4) == 0 and ops.prototype_workspace(1, 4, 2, 1024, 1025) == 0


def test_module_validates_on_the_host():
    from weaklysuperviseddl_amd import ops, nn as wnn
    crit = wnn.PrototypeContrastLoss(2, source="bank")
    assert crit.bank is None and crit.count is None and "source='bank'" in repr(crit) and not list(crit.parameters())
    crit.reset()
    assert set(dict(crit.named_buffers())) == set() and list(crit.state_dict()) == []          # nothing before the first call
    saved = {"bank": torch.arange(8.0).view(2, 4), "count": torch.tensor([3, 0])}
    crit.load_state_dict(saved)                                                             # the bank is a registered buffer
    assert torch.equal(crit.bank, saved["bank"]) and torch.equal(crit.count, saved["count"]) and crit.count.dtype == torch.int64
    assert sorted(crit.state_dict()) == ["bank", "count"] and sorted(dict(crit.named_buffers())) == ["bank", "count"]
    twin = wnn.PrototypeContrastLoss(2, source="bank")
    twin.load_state_dict(crit.state_dict())
    assert torch.equal(twin.bank, crit.bank) and twin.bank is not crit.bank and crit.double().bank.dtype == torch.float64
    for args in ((0,), (33,), (2, 0.0), (2, 0.1, "dataset"), (2, 0.1, "bank", 1.5)):
        with pytest.raises(ops.WsdlError):
            wnn.PrototypeContrastLoss(*args)
    with pytest.raises(ops.WsdlError):
        crit(torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int64))          # host tensors: no CPU fallback


def test_generate_prototype_pseudo_masks_refuses_combinations():
    """The prototype option lives in a function of its own: the signature of generate_pseudo_masks is pinned
    (tests/test_multiscale.py) and stays as it was."""
    import inspect
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import generate_prototype_pseudo_masks, generate_pseudo_masks
    assert "prototype" not in inspect.signature(generate_pseudo_masks).parameters
    net = object()
    for kw in (dict(pamr={}), dict(superpixels=dict(step=8)), dict(affinity=dict(net=net)), dict(boundary=dict(net=net))):
        with pytest.raises(ValueError, match="prototype"):
            generate_prototype_pseudo_masks([], None, dict(net=net), write_png=False, **kw)
    for proto in ({}, dict(lo=0.1), dict(net=net, radius=3), [net], dict(net=net, lo=0.5, hi=0.5)):
        with pytest.raises(ValueError):
            generate_prototype_pseudo_masks([], None, proto, write_png=False)
    for proto in (dict(net=net, temperature=0.0), dict(net=net, temperature=float("nan"))):
        with pytest.raises(ops.WsdlError):
            generate_prototype_pseudo_masks([], None, proto, write_png=False)
    with pytest.raises(TypeError):
        generate_prototype_pseudo_masks([], None, dict(net=net), thresh=0.3)                        # not a keyword of generate_pseudo_masks
    generate_prototype_pseudo_masks([], None, dict(net=net), multiscale=None, write_png=False)      # an empty loader: nothing runs
    assert generate_pseudo_masks.last_masks == []


def test_projection_net_parameters():
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM, ProjectionNet, TrunkFeatures, train_projection_net
    net = ProjectionNet(FrozenResNetCAM(37), dim=32)
    head = {k: tuple(p.shape) for k, p in net.named_parameters() if p.requires_grad}
    assert head == {"f8_3.weight": (64, 512, 1, 1), "f8_4.weight": (128, 1024, 1, 1), "f8_5.weight": (256, 2048, 1, 1),
                    "proj.weight": (32, 448, 1, 1)}
    assert all(k.startswith("trunk.") for k, p in net.named_parameters() if not p.requires_grad)
    assert {k for k in net.state_dict() if not k.startswith("trunk.")} == set(head)
    assert len(net.head_parameters()) == 4 and not net.train().trunk.training and net.training
    assert ProjectionNet(FrozenResNetCAM(37)).proj.weight.shape[0] == 128
    tf = TrunkFeatures(FrozenResNetCAM(37), "layer3")
    assert not [p for p in tf.parameters() if p.requires_grad] and not tf.train().trunk.training
    for bad in (dict(dim=0), dict(dim=4096), dict(dim=1.5)):
        with pytest.raises(ValueError):
            ProjectionNet(FrozenResNetCAM(37), **bad)
    with pytest.raises(ValueError):
        TrunkFeatures(FrozenResNetCAM(37), "layer1")
    cams = [torch.zeros(1, 8, 8)]
    for kw in (dict(epochs=0), dict(lo=0.5, hi=0.5), dict(cams=3)):
        with pytest.raises(ValueError):
            train_projection_net(net, [], **dict(dict(cams=cams, device="cpu", log=None), **kw))
    with pytest.raises(ValueError):
        train_projection_net(object(), [], cams, device="cpu", log=None)
    from weaklysuperviseddl_amd import ops
    for kw in (dict(temperature=0.0), dict(source="dataset"), dict(momentum=2.0)):
        with pytest.raises(ops.WsdlError):
            train_projection_net(net, [], cams, device="cpu", log=None, **kw)
