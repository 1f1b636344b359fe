"""Multi-scale + flip fusion on the device (csrc/multiscale.hip) against the oracle of tests/multiscale_oracle.py.

Parity bound (the project's standing one): the oracle run in float32 on the CPU with the device's operation order, against
its float64 run, is the yardstick, computed per case and combination; a device score may be at most
``max(4 x yardstick, 2^-23 |value|)`` from float64, plus ONE derived term, ``mo.fused_coordinate_term``:

  The contract demands ``wsdl_bilinear_fwd``'s bits, and that kernel forms the source coordinate ``scale * (o + 0.5) - 0.5`` with
  one rounding (a fused multiply-add).  Below 1/2 - everywhere on a one-pixel axis, at the first output pixels otherwise - the
  weight ``l1`` then has more than 24 bits and ``l0 = 1 - l1`` is rounded: ``l0 + l1 = 1 + d``, ``|d| <= 2^-25`` per axis.  The
  float32 oracle's unfused coordinate is a multiple of 2^-24 there, its ``l0 + l1`` is exactly 1, and on EQUAL taps (a 1 x 1
  source, a clamped border) its two rounded products sum to within half an ulp of the tap and round back to it: the oracle is
  exact, its yardstick 0 (case 12: 1.5e-8 on one channel, 0 on the others), where the device's ``v (1 + d)`` plus the same
  product roundings may land one ulp off at each of the two lerp levels and the second level's roundings add less than one more.
  Hence ``3 * 2^-23 A`` with A the largest tap magnitude of the plane, times the activation's Lipschitz constant (none 1,
  sigmoid 1/4, softmax 1/2 with A over all channels); means and maxima over members do not enlarge it.  The factor 4 stays.
  Measured without the term: every case but that one was inside ``max(4 x yardstick, 2^-23 |value|)`` (worst ratio 0.73), case 12
  read 4.8e-7 = 2 ulp at the value 1.98 against 2.4e-7.

Elsewhere the device and the float32 oracle round the same coordinate (the error that dominates both: up to 1e-4 of a logit
step at a 400-wide source) and combine the members in double.  Labels are compared where the float64 top-two margin exceeds twice that bound,
which may leave out at most 0.1 % of a case's pixels (tests/test_multiscale.py asserts the same of the float32 oracle).  The
worst device-error-to-bound ratio of every case is reported with ``report_line``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiscale_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def run_case(ops, dev, case, combo, **kw):
    (H, W), _sizes, mirrored, _B, _C = mo.GEOMETRIES[case]
    act, red, weighted = combo
    srcs = [s.to(dev) for s in mo.reference(case)["sources"]]
    return ops.multiscale_fuse(srcs, (H, W), mirrored=list(mirrored), weights=mo.case_weights(case) if weighted else None,
                               activation=act, reduce=red, **kw)


@pytest.mark.parametrize("case", range(len(mo.GEOMETRIES)))
def test_scores_against_float64(dev, case):
    """Every activation x reduce x weights of the case: scores within the bound of float64; labels and conf of the same launch
    are ``pamr_labels`` of the returned scores exactly; a second call gives the same bits."""
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    ref = mo.reference(case)
    worst = (0.0, None)
    for combo, r in ref["combos"].items():
        scores, labels, conf = run_case(ops, dev, case, combo, labels=True, conf=True, min_conf=0.3, thresh=0.25)
        assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.grad_fn is None
        assert tuple(scores.shape) == tuple(r["r64"].shape) and labels.dtype == torch.int64 and conf.dtype == torch.float32
        err = (scores.cpu().double() - r["r64"]).abs()
        limit = mo.bound(r["r64"], r["yard"], mo.fused_coordinate_term(case, combo[0]))
        ratio = (err / limit.clamp(min=1e-300)).max().item()
        print(f"case {case} {combo}: max |device - float64| {err.max().item():.3e}, float32 oracle {r['yard']:.3e}, error / bound {ratio:.3f}")
        if ratio > worst[0]:
            worst = (ratio, combo)
        assert (err <= limit).all(), (case, combo, err.max().item(), r["yard"], ratio)
        if scores.shape[1] <= 32:
            assert torch.equal(labels, ops.pamr_labels(scores, thresh=0.25, min_conf=0.3))
        else:               # pamr_labels takes up to 32 channels: its rule as the oracle restates it
            assert torch.equal(labels.cpu(), mo.labels(scores.cpu(), thresh=0.25, min_conf=0.3)[0])
        want_conf = scores[:, 0] if scores.shape[1] == 1 else scores.amax(dim=1)
        assert torch.equal(conf, want_conf)
        again = run_case(ops, dev, case, combo)
        assert torch.equal(again, scores)
    (H, W), sizes, mirrored, B, C = mo.GEOMETRIES[case]
    report_line(f"multiscale_fuse {B}x{C}x{H}x{W} from {len(sizes)} source(s), {sum(mirrored)} mirrored: worst device error / bound "
                f"{worst[0]:.3f} ({worst[1]})")


@pytest.mark.parametrize("case", range(len(mo.GEOMETRIES)))
def test_labels_against_float64(dev, case):
    """A labels-only launch (no score planes) equals the labels of the full launch, and the float64 oracle's labels wherever its
    top-two margin exceeds twice the bound; at most 0.1 % of the pixels are left out (``mo.label_combos``)."""
    from weaklysuperviseddl_amd import ops
    ref = mo.reference(case)["combos"]
    for combo in mo.label_combos(mo.GEOMETRIES[case][4]):
        r = ref[combo]
        labels = run_case(ops, dev, case, combo, scores=False, labels=True)
        full = run_case(ops, dev, case, combo, labels=True, conf=True)
        assert labels.dtype == torch.int64 and torch.equal(labels, full[1])
        sure = mo.label_margin(r["r64"]) > 2 * mo.bound(r["r64"], r["yard"], mo.fused_coordinate_term(case, combo[0])).amax(dim=1)
        assert (~sure).double().mean().item() <= 1e-3
        want, _ = mo.labels(r["r64"])
        assert torch.equal(labels.cpu()[sure], want[sure]), (case, combo)


def test_scale_flip_equals_bilinear_resize_and_its_mirror(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(1)
    for (B, C, H, W), (h, w) in (((2, 3, 17, 23), (32, 32)), ((1, 1, 64, 64), (96, 160)), ((3, 2, 40, 30), (13, 7)), ((2, 3, 8, 9), (8, 9)),
                                 ((1, 2, 1, 1), (5, 4)), ((1, 1, 33, 70), (1, 1)), ((1, 4, 3, 300), (7, 129))):
        x = torch.randn(B, C, H, W, generator=g).to(dev)
        keep = x.clone()
        want = ops.bilinear_resize(x, (h, w))
        plain = ops.scale_flip(x, (h, w))
        assert torch.equal(plain, want) and plain.grad_fn is None
        both = ops.scale_flip(x, (h, w), flip=True)
        assert tuple(both.shape) == (2 * B, C, h, w) and torch.equal(both[:B], want) and torch.equal(both[B:], want.flip(-1))
        out = torch.full_like(both, float("nan"))
        assert ops.scale_flip(x, (h, w), flip=True, out=out) is out and torch.equal(out, both)
        assert torch.equal(x, keep)
        # a strided input is copied, the result is that of the dense tensor
        wide = torch.randn(B, C, H, W + 3, generator=g).to(dev)
        assert torch.equal(ops.scale_flip(wide[..., 1:W + 1], (h, w), True), ops.scale_flip(wide[..., 1:W + 1].contiguous(), (h, w), True))
    with pytest.raises(ops.WsdlError):
        ops.scale_flip(x, (7, 129), out=torch.empty(1, 4, 7, 128, device=dev))


def test_one_plain_source_is_bilinear_resize(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(2)
    for (B, C, h, w), (H, W) in (((2, 3, 8, 8), (64, 64)), ((1, 21, 12, 17), (96, 130)), ((1, 64, 5, 4), (37, 53)), ((3, 1, 40, 90), (5, 7)),
                                 ((1, 2, 1, 1), (3, 300)), ((2, 30, 9, 9), (9, 9))):
        x = torch.randn(B, C, h, w, generator=g).to(dev)
        assert torch.equal(ops.multiscale_fuse([x], (H, W)), ops.bilinear_resize(x, (H, W))), (B, C, h, w, H, W)
        assert torch.equal(ops.multiscale_fuse(x, (H, W), reduce="max"), ops.bilinear_resize(x, (H, W)))


def test_direct_read_keeps_an_infinity(dev):
    """A source of the target's size is read, not interpolated with a zero weight: inf stays inf (0 * inf would be NaN)."""
    from weaklysuperviseddl_amd import ops
    for C in (2, 30):
        x = torch.zeros(1, C, 6, 7, device=dev)
        x[0, 1, 2, 3] = float("inf")
        x[0, 0, 5, 6] = float("-inf")
        small = torch.ones(1, C, 2, 2, device=dev)
        for red in ("mean", "max"):
            one = ops.multiscale_fuse([x], (6, 7), reduce=red)
            assert torch.equal(one, x)
            two = ops.multiscale_fuse([x, small], (6, 7), reduce=red)
            assert two[0, 1, 2, 3].item() == float("inf") and torch.isfinite(two[0, 1, 2, 2]).item()
            assert not torch.isnan(two).any()
        both = torch.cat([x, x.flip(-1)])
        assert torch.equal(ops.multiscale_fuse([both], (6, 7), mirrored=True), x)


def test_labels_rule_ties_nan_and_threshold(dev):
    from weaklysuperviseddl_amd import ops
    s = torch.tensor([[[[0.2, 0.5, float("nan"), 0.1]], [[0.2, 0.4, 0.3, 0.3]], [[0.1, 0.5, 0.9, 0.05]]]], device=dev)
    scores, labels, conf = ops.multiscale_fuse([s], (1, 4), labels=True, conf=True, min_conf=0.3)
    assert labels.flatten().tolist() == [255, 0, 0, 1] and torch.equal(labels, ops.pamr_labels(scores, min_conf=0.3))
    assert conf.flatten().tolist()[:2] == pytest.approx([0.2, 0.5]) and conf.flatten().tolist()[3] == pytest.approx(0.3)
    assert ops.multiscale_fuse([s], (1, 4), scores=False, labels=True, min_conf=0.3, ignore_index=-7).flatten().tolist() == [-7, 0, 0, 1]
    one = torch.tensor([0.5, 0.4999, float("nan"), 0.6], device=dev).view(1, 1, 2, 2)
    sc, lab, cf = ops.multiscale_fuse([one], (2, 2), labels=True, conf=True, thresh=0.5, min_conf=0.9)
    assert lab.flatten().tolist() == [1, 0, 0, 1] and torch.equal(lab, ops.pamr_labels(sc, thresh=0.5, min_conf=0.9))
    assert torch.equal(cf.nan_to_num(9.0), one[:, 0].nan_to_num(9.0))
    # 30 channels (the two-pass kernel): a NaN pixel and a tie
    big = torch.zeros(1, 30, 1, 3, device=dev)
    big[0, 7, 0, 0] = big[0, 9, 0, 0] = 2.0
    big[0, 4, 0, 1] = float("nan")
    big[0, 29, 0, 2] = 1.0
    sc, lab = ops.multiscale_fuse([big], (1, 3), labels=True)
    assert lab.flatten().tolist() == [7, 0, 29] and torch.equal(lab, ops.pamr_labels(sc))
    out = {"labels": torch.empty(1, 1, 3, dtype=torch.int64, device=dev)}
    assert ops.multiscale_fuse([big], (1, 3), scores=False, labels=True, out=out) is out["labels"]


def test_strided_sources_are_handled(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(4)
    wide = torch.randn(4, 5, 9, 14, generator=g).to(dev)
    view = wide[:, 1:4, :, 2:13]
    assert not view.is_contiguous()
    got = ops.multiscale_fuse([view], (20, 31), mirrored=True, activation="softmax")
    assert torch.equal(got, ops.multiscale_fuse([view.contiguous()], (20, 31), mirrored=True, activation="softmax"))


def test_mirror_image_of_a_source_is_undone(dev):
    """A source and its own mirror image fused with ``mirrored``: at the target's size exactly the source; at other sizes within
    the bound of the fusion of the source alone in float64 (an off-by-one mirror index would be a whole pixel off), at odd
    and even widths."""
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(5)
    for (h, w), (H, W) in (((6, 9), (6, 9)), ((6, 8), (6, 8)), ((6, 9), (13, 20)), ((6, 8), (13, 21)), ((7, 5), (3, 4)), ((9, 12), (40, 33))):
        x = torch.randn(2, 3, h, w, generator=g)
        both = torch.cat([x, x.flip(-1)]).to(dev)
        got = ops.multiscale_fuse([both], (H, W), mirrored=True)
        if (h, w) == (H, W):
            assert torch.equal(got.cpu(), x)
            continue
        want64 = mo.fuse([x], (H, W))
        yard = (mo.fuse([both.cpu()], (H, W), mirrored=True, dtype=torch.float32).double() - want64).abs().max().item()
        assert yard > 0
        assert ((got.cpu().double() - want64).abs() <= mo.bound(want64, yard)).all()


def test_max_normalize(dev):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(7, 2, 37, 53, generator=g)
    x[1] = 0.0
    x[2] = -x[2].abs() - 0.1
    x[3, 0, 5, 5] = float("nan")
    x[4, 1, 0, 0] = float("inf")
    x[5] = x[5].abs() * 1e-30
    want, want_mask = mo.max_normalize(x, 0.3)
    xd = x.to(dev)
    keep = xd.clone()
    out, mask = ops.max_normalize(xd, 0.3)
    assert torch.equal(out.cpu().nan_to_num(7.0), want.nan_to_num(7.0)) and torch.equal(mask.cpu(), want_mask)
    assert mask.dtype == torch.uint8 and torch.equal(xd.nan_to_num(7.0), keep.nan_to_num(7.0))
    for b in (1, 2, 3, 4):
        assert torch.equal(out[b].nan_to_num(7.0), xd[b].nan_to_num(7.0))               # untouched
    assert out[0].max().item() == 1.0 and out[5].max().item() == 1.0 and out[6].max().item() == 1.0
    assert not mask[1].any() and not mask[2].any()                                      # v >= thresh && v > 0
    zero_thresh = ops.max_normalize(xd, 0.0)[1]
    assert torch.equal(zero_thresh.cpu(), ((want >= 0) & (want > 0)).to(torch.uint8))
    again = ops.max_normalize(xd)
    assert torch.equal(again.nan_to_num(7.0), out.nan_to_num(7.0))
    inplace = xd.clone()
    assert ops.max_normalize(inplace, out=inplace) is inplace and torch.equal(inplace.nan_to_num(7.0), out.nan_to_num(7.0))
    big = torch.rand(1, 1, 300, 1000, generator=g).to(dev)                              # many workgroups per image
    assert torch.equal(ops.max_normalize(big).cpu(), mo.max_normalize(big.cpu()))


def test_a_launch_plan_replays_scale_flip_and_the_fusion(dev):
    from weaklysuperviseddl_amd import ops, plan
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 24, 40, generator=g).to(dev)
    other = torch.randn(2, 3, 5, 9, generator=g).to(dev)
    out = {}

    def seq():
        a = ops.scale_flip(x, (12, 20), flip=True)
        b = ops.scale_flip(x, (30, 50), flip=True)
        return ops.multiscale_fuse([a, other, b], (24, 40), mirrored=[True, False, True], weights=[1.0, 0.5, 2.0], activation="softmax",
                                   labels=True, conf=True, out=out)

    p, res = plan.record(seq)
    assert p.stats["kernels"] == 3 and res[0] is out["scores"]
    x.copy_(torch.randn(2, 3, 24, 40, generator=g).to(dev))
    other.copy_(torch.randn(2, 3, 5, 9, generator=g).to(dev))
    first = [t.clone() for t in res]
    p.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in res]
    out2 = {}
    a = ops.scale_flip(x, (12, 20), flip=True)
    b = ops.scale_flip(x, (30, 50), flip=True)
    eager = ops.multiscale_fuse([a, other, b], (24, 40), mirrored=[True, False, True], weights=[1.0, 0.5, 2.0], activation="softmax",
                                labels=True, conf=True, out=out2)
    assert all(torch.equal(r, e) for r, e in zip(replayed, eager)) and not torch.equal(replayed[0], first[0])


@pytest.fixture(scope="module")
def seg_model(dev):
    from weaklysuperviseddl_amd import nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model
    torch.manual_seed(0)
    model = build_segmentation_model()
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if isinstance(mod, wnn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return model.to(dev).eval()


def test_predict_multiscale_is_the_composition_of_the_ops(dev, seg_model):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import predict_multiscale
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    scales = (0.5, 1.0, 1.5)
    assert ops.multiscale_sizes(64, 64, scales) == [(32, 32), (64, 64), (96, 96)]
    labels, scores = predict_multiscale(seg_model, x, scales, True, scores=True)
    with torch.no_grad():
        srcs = [seg_model.head_logits(ops.scale_flip(x, s, True)) for s in ops.multiscale_sizes(64, 64, scales)]
    assert [tuple(s.shape) for s in srcs] == [(4, 2, 4, 4), (4, 2, 8, 8), (4, 2, 12, 12)]
    want_scores, want_labels = ops.multiscale_fuse(srcs, (64, 64), mirrored=True, activation="softmax", labels=True)
    assert torch.equal(scores, want_scores) and torch.equal(labels, want_labels) and labels.dtype == torch.int64
    assert torch.equal(predict_multiscale(seg_model, x, scales, True), labels)
    assert (scores.sum(dim=1) - 1).abs().max().item() < 1e-6 and not seg_model.training
    # one scale, no mirror image, no activation: the network's own output, bit for bit
    with torch.no_grad():
        plain = seg_model(x)["out"]
        assert torch.equal(ops.bilinear_resize(seg_model.head_logits(x), (64, 64)), plain)
    lab1, sc1 = predict_multiscale(seg_model, x, (1.0,), False, activation="none", scores=True)
    assert torch.equal(sc1, plain) and torch.equal(lab1, plain.argmax(dim=1))
    # a model without head_logits is asked for its ['out']

    class Wrapped(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, t):
            return {"out": self.m.head_logits(t)}
    assert torch.equal(predict_multiscale(Wrapped(seg_model).eval(), x, scales, True), labels)
    seg_model.train()
    try:
        assert torch.equal(predict_multiscale(seg_model, x, scales, True), labels) and seg_model.training
    finally:
        seg_model.eval()


def test_evaluate_model_with_and_without_scales(dev, seg_model):
    import oracle
    from weaklysuperviseddl_amd.TraditionalModel import evaluate_model, predict_multiscale
    g = torch.Generator().manual_seed(9)
    loader = []
    for hw in ((64, 64), (96, 80), (48, 56)):
        img = torch.randn(2, 3, 64, 64, generator=g)
        loader.append((img, (torch.zeros(2, dtype=torch.long), torch.randint(1, 4, (2,) + hw, generator=g))))

    def by_hand(predict, mode):
        ious, accs = [], []
        for img, (_, tm) in loader:
            t = tm[0].clone()
            if mode == "notebook":
                t[t == 2] = 1
                t = 1 - t
            else:
                t = (t == 1).long()
            pred = predict(img[0:1].to(dev)).cpu()
            if pred.shape != t.shape:
                pred = torch.nn.functional.interpolate(pred[None, None].float(), size=t.shape[-2:], mode="nearest").squeeze().long()
            iou, acc = oracle.compute_iou_and_acc(pred, t)
            ious.append(iou)
            accs.append(acc)
        return sum(ious) / len(ious), sum(accs) / len(accs)

    for mode in ("notebook", "modular"):
        with torch.no_grad():
            old = by_hand(lambda t: seg_model(t)["out"].argmax(dim=1)[0], mode)
        assert evaluate_model(seg_model, loader, dev, mode) == pytest.approx(old, abs=1e-6)          # the old positional call
        new = by_hand(lambda t: predict_multiscale(seg_model, t, (0.5, 1.0, 1.5), True)[0], mode)
        assert evaluate_model(seg_model, loader, dev, mode, scales=(0.5, 1.0, 1.5), flip=True) == pytest.approx(new, abs=1e-6)
        flip_only = by_hand(lambda t: predict_multiscale(seg_model, t, (1.0,), True)[0], mode)
        assert evaluate_model(seg_model, loader, dev, mode, flip=True) == pytest.approx(flip_only, abs=1e-6)


@pytest.fixture(scope="module")
def cam_gen(dev):
    from weaklysuperviseddl_amd.TraditionalModel import FrozenResNetCAM, LayerCAMGenerator
    torch.manual_seed(0)
    model = FrozenResNetCAM(37)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return LayerCAMGenerator(model.to(dev).eval(), ["layer3", "layer4"], out_hw=(64, 64))


def test_generate_multiscale_is_the_composition_of_the_ops(dev, cam_gen):
    from weaklysuperviseddl_amd import ops
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 3, 64, 64, generator=g).to(dev)
    cls = torch.tensor([3, 11], device=dev)
    scales = (0.5, 1.0, 1.5)
    for reduce in ("mean", "max"):
        cam, mask = cam_gen.generate_multiscale(x, scales, True, 1.0, cls, thresh=0.3, reduce=reduce)
        cams = [cam_gen._generate_batch_eager(ops.scale_flip(x, s, True), 1.0, torch.cat([cls, cls]), None)[:, None]
                for s in ((32, 32), (64, 64), (96, 96))]
        assert all(tuple(c.shape) == (4, 1, 64, 64) for c in cams)
        want, want_mask = ops.max_normalize(ops.multiscale_fuse(cams, (64, 64), mirrored=True, reduce=reduce), 0.3)
        assert torch.equal(cam, want[:, 0]) and torch.equal(mask, want_mask[:, 0]) and tuple(cam.shape) == (2, 64, 64)
        assert cam.amax(dim=(1, 2)).tolist() == [1.0, 1.0] and 0 < int(mask.sum()) < mask.numel()
        assert torch.equal(cam_gen.generate_multiscale(x, scales, True, 1.0, cls, reduce=reduce), cam)
    no_flip = cam_gen.generate_multiscale(x, (1.0,), False, 1.0, cls)
    single = cam_gen._generate_batch_eager(x, 1.0, cls, None)
    assert torch.equal(no_flip, ops.max_normalize(single[:, None])[:, 0])


def test_generate_pseudo_masks_multiscale(dev, cam_gen):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import generate_pseudo_masks
    g = torch.Generator().manual_seed(41)
    loader = [(torch.rand(2, 3, 64, 64, generator=g), (torch.tensor([3, 11]), None))]
    kw = dict(cam_thresh=0.3, write_png=False, max_images=2, device_batch=0, keep_on_device=True)
    generate_pseudo_masks(loader, cam_gen, **kw)
    plain = [t.clone() for t in generate_pseudo_masks.last_masks]
    generate_pseudo_masks(loader, cam_gen, multiscale=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, generate_pseudo_masks.last_masks)) and len(plain) == 2
    ms = dict(scales=(0.5, 1.0, 1.5), flip=True)
    generate_pseudo_masks(loader, cam_gen, multiscale=ms, **kw)
    got = torch.stack(generate_pseudo_masks.last_masks)
    imgs, cls = loader[0][0].to(dev), loader[0][1][0].to(dev)
    cam, mask = cam_gen.generate_multiscale(imgs, alpha=1.0, class_idx=cls, thresh=0.3, **ms)
    assert torch.equal(got, ops.keep_largest_batched(mask)) and 0 < int(got.sum()) < got.numel()
    # the fused CAM takes the CAM's place in front of a refinement
    generate_pseudo_masks(loader, cam_gen, multiscale=ms, pamr=dict(num_iter=2, dilations=(1, 2)), **kw)
    want = ops.keep_largest_batched(ops.pamr_labels(ops.pamr(imgs, cam[:, None], num_iter=2, dilations=(1, 2)), thresh=0.3).to(torch.uint8))
    assert torch.equal(torch.stack(generate_pseudo_masks.last_masks), want)
    with pytest.raises(ValueError, match="device_batch"):
        generate_pseudo_masks(loader, cam_gen, multiscale=ms, **dict(kw, device_batch=8))
