"""Distance transforms, boundary bands, Boundary IoU counts, the boundary confidence map and the boundary-aware criterion on
the device (csrc/edt.hip) against the brute-force oracle of tests/edt_oracle.py.

Distances, bands and counts are integers: equal, never close.  Confidence parity bound: the SAME oracle run in torch float32
on the CPU against its float64 run is the yardstick, computed here per case; the device may be at most 4 x that (the margin
tests/test_hip_pamr.py uses for a different ``exp``; there is no summation here).  The worst device values are reported
with ``report_line``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [(m, b) for m in eo.METRICS for b in (False, True)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case, value=1):
    """Labels of one case and the oracle's planes for every metric / border - computed once, shared, never written."""
    B, H, W = eo.CASES[case]
    labels = eo.make_labels(B, H, W, 300 + case)
    return labels, {(m, b): eo.dist2(labels, value, m, b) for m, b in COMBOS}


def same(plane, want):
    return plane.dtype == torch.int32 and plane.is_contiguous() and torch.equal(plane.cpu().long(), want)


def check_against_oracle(dev, labels, value=1, combos=COMBOS):
    from weaklysuperviseddl_amd import ops
    on_dev = labels.to(dev)
    for metric, border in combos:
        want_out, want_in = eo.dist2(labels, value, metric, border)
        d_out, d_in = ops.edt(on_dev, value, metric=metric, border=border)
        assert same(d_out, want_out), (metric, border, "out")
        assert same(d_in, want_in), (metric, border, "in")


# ------------------------------------------------------------------------------------------------------ 1. exact distances
@pytest.mark.parametrize("case", range(len(eo.CASES)))
def test_distances_are_exact(dev, case):
    from weaklysuperviseddl_amd import ops
    labels, ref = reference(case)
    on_dev = labels.to(dev)
    for (metric, border), (want_out, want_in) in ref.items():
        d_out, d_in = ops.edt(on_dev, metric=metric, border=border)
        assert same(d_out, want_out), (eo.CASES[case], metric, border, "out")
        assert same(d_in, want_in), (eo.CASES[case], metric, border, "in")
    assert torch.equal(on_dev.cpu(), labels)                             # the input is never written


# ------------------------------------------------------------------------------------------------------ 2. special contents
def test_all_in_and_all_out_images(dev):
    from weaklysuperviseddl_amd import ops
    ones = torch.ones(2, 9, 70, dtype=torch.int64)
    for metric in eo.METRICS:
        d_out, d_in = ops.edt(ones.to(dev), metric=metric)
        assert (d_out == ops.EDT_FAR).all() and (d_in == 0).all()
        d_out, d_in = ops.edt(ones.to(dev), 0, metric=metric, border=True)          # value 0: every pixel is OUT
        assert (d_out == 0).all() and (d_in == ops.EDT_FAR).all()
    check_against_oracle(dev, ones)                                      # border=True: the distance to the outside
    check_against_oracle(dev, ones, value=0)


def test_corner_pixel_checkerboard_and_lines(dev):
    corner = torch.zeros(1, 33, 47, dtype=torch.int64)
    corner[0, 32, 46] = 1
    yy, xx = torch.meshgrid(torch.arange(10), torch.arange(67), indexing="ij")
    checker = ((yy + xx) % 2)[None].contiguous()
    lines = torch.zeros(2, 40, 90, dtype=torch.int64)
    lines[0, 17, :] = 1                                                  # a full row
    lines[1, 3:38, 61] = 1                                               # a column segment
    for labels in (corner, checker, lines):
        check_against_oracle(dev, labels)


def test_value_two_bool_input_and_a_null_plane(dev):
    from weaklysuperviseddl_amd import ops
    labels, _ = reference(4)
    assert set(labels.unique().tolist()) == {0, 1, 2, 255}
    check_against_oracle(dev, labels, value=2)
    check_against_oracle(dev, labels, value=255, combos=COMBOS[:1])
    # a bool / uint8 mask is converted
    want = ops.edt(labels.to(dev))
    for mask in ((labels == 1).to(dev), (labels == 1).to(torch.uint8).to(dev)):
        got = ops.edt(mask)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a plane that is not wanted is neither returned nor written
    poison = torch.full(tuple(labels.shape), -7, dtype=torch.int32, device=dev)
    bufs = {"out": torch.empty(tuple(labels.shape), dtype=torch.int32, device=dev), "in": poison}
    d_out, d_in = ops.edt(labels.to(dev), want=("out",), out=bufs)
    assert d_in is None and d_out is bufs["out"] and torch.equal(d_out, want[0]) and (poison == -7).all()
    d_out, d_in = ops.edt(labels.to(dev), want="in", metric="chebyshev")
    assert d_out is None and same(d_in, eo.dist2(labels, 1, "chebyshev")[1])


# ------------------------------------------------------------------------------------------------------ 3. reproducibility
def test_out_buffers_are_reused_and_refusals(dev):
    from weaklysuperviseddl_amd import ops
    labels, ref = reference(4)
    on_dev = labels.to(dev)
    bufs = {}
    a = ops.edt(on_dev, border=True, out=bufs)
    first = [t.clone() for t in a]
    ptrs = [t.data_ptr() for t in a]
    b = ops.edt(on_dev, border=True, out=bufs)
    assert [t.data_ptr() for t in b] == ptrs and b[0] is bufs["out"] and b[1] is bufs["in"]
    assert torch.equal(b[0], first[0]) and torch.equal(b[1], first[1]) and same(b[0], ref[("euclid", True)][0])
    with pytest.raises(ops.WsdlError):
        ops.edt(torch.zeros(1, 0, 4, dtype=torch.int64, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.edt(torch.zeros(1, 8193, 1, dtype=torch.int64, device=dev))
    with pytest.raises(ops.WsdlError):
        ops.edt(torch.zeros(1, 4, 4, device=dev))                         # float labels
    with pytest.raises(ops.WsdlError):
        ops.edt(torch.zeros(4, 4, dtype=torch.int64, device=dev))         # not (B,H,W)


# ------------------------------------------------------------------------------------------------------ 4. bands and counts
@pytest.mark.parametrize("case", (3, 4, 5))
def test_boundary_band_equals_the_erosion(dev, case):
    from weaklysuperviseddl_amd import ops
    labels, _ = reference(case)
    for width in (1, 2, 5):
        got = ops.boundary_band(labels.to(dev), width)
        assert got.dtype == torch.bool and torch.equal(got.cpu(), eo.band(labels == 1, width)), width
    assert torch.equal(ops.boundary_band(labels.to(dev), 2, value=2).cpu(), eo.band(labels == 2, 2))


def count_batch():
    """(4,37,53): two different blob images; an image where neither map has a pixel of the class (both bands empty); a 2 x 2
    object against its shifted self (with width 5 the band is the whole object)."""
    labels = eo.make_labels(4, 37, 53, 41)
    preds = eo.make_labels(4, 37, 53, 42)
    preds[0] = torch.roll(labels[0], (2, -3), (0, 1))                    # an overlapping prediction
    labels[1][labels[1] == 1] = 0
    preds[1][preds[1] == 1] = 2
    labels[2].zero_()
    preds[2].zero_()
    labels[2, 10:12, 20:22] = 1
    preds[2, 10:12, 21:23] = 1
    return preds, labels


def test_boundary_iou_counts_are_exact_per_image(dev):
    from weaklysuperviseddl_amd import ops
    preds, labels = count_batch()
    for width in (1, 5):
        want = eo.boundary_iou_counts(preds, labels, width)
        got = ops.boundary_iou_counts(preds.to(dev), labels.to(dev), width)
        assert got.dtype == torch.int64 and tuple(got.shape) == (4, 2) and got.tolist() == [list(c) for c in want], width
        assert want[1] == (0, 0) and want[0][0] > 0
        assert ops.boundary_iou_from_counts(got.cpu().numpy()) == eo.mean_iou(want)
        assert ops.boundary_iou_from_counts(got.cpu().numpy(), EMPTY=0.0) == eo.mean_iou(want, EMPTY=0.0)
    assert eo.boundary_iou_counts(preds, labels, 5)[2] == (2, 6)         # the band covers the whole 2 x 2 object
    row = torch.full((4, 2), -1, dtype=torch.int64, device=dev)           # overwritten, not accumulated
    assert ops.boundary_iou_counts(preds.to(dev), labels.to(dev), 1, out=row) is row
    assert row.tolist() == [list(c) for c in eo.boundary_iou_counts(preds, labels, 1)]


@pytest.mark.parametrize("ratio", (0.02, 0.1))
def test_boundary_iou_equals_the_published_definition(dev, ratio):
    from weaklysuperviseddl_amd import ops
    labels = eo.make_labels(4, 37, 53, 51)
    preds = torch.roll(labels, (1, 2), (1, 2))
    preds[3] = eo.make_labels(1, 37, 53, 52)[0]
    want = eo.boundary_iou(preds, labels, ratio)
    got = ops.boundary_iou(preds.to(dev), labels.to(dev), ratio)
    print(f"Boundary IoU at ratio {ratio} (width {eo.boundary_width(37, 53, ratio)}): device {got!r}, oracle {want!r}")
    assert isinstance(got, float) and got == want and 0.0 < want < 1.0
    assert ops.boundary_iou(labels.to(dev), labels.to(dev), ratio) == 1.0


def test_boundary_iou_on_hand_made_cases(dev):
    """The 8 x 8 cases worked out in tests/test_edt.py: 6/18, 12/12, 0/0, 7/33."""
    from weaklysuperviseddl_amd import ops
    from test_edt import hand_cases
    p, g, want = hand_cases()
    assert ops.boundary_iou_counts(p.to(dev), g.to(dev), 1).tolist() == [list(c) for c in want]
    assert ops.boundary_iou(p.to(dev), g.to(dev), width=1) == (1.0 / 3.0 + 1.0 + 1.0 + 7.0 / 33.0) / 4


# ------------------------------------------------------------------------------------------------------ 5. confidence
@pytest.mark.parametrize("case,sigma,floor", ((4, 3.0, 0.0), (4, 1.7, 0.25), (5, 3.0, 0.1), (7, 0.8, 0.0)))
def test_confidence_against_float64(dev, case, sigma, floor):
    from conftest import report_line
    from weaklysuperviseddl_amd import ops
    labels, ref = reference(case)
    d_out, d_in = ref[("euclid", False)]
    w64 = eo.confidence(d_out, d_in, sigma, floor)
    w32 = eo.confidence(d_out, d_in, sigma, floor, dtype=torch.float32)
    assert w32.dtype == torch.float32
    yard = (w32.double() - w64).abs().max().item()
    w = ops.boundary_confidence(labels.to(dev), sigma, floor)
    err = (w.cpu().double() - w64).abs().max().item()
    shape = "x".join(str(v) for v in eo.CASES[case])
    report_line(f"boundary confidence {shape} sigma={sigma} floor={floor}: max |device - float64| {err:.2e} (float32 oracle {yard:.2e})")
    print(f"confidence {shape}: device {err:.3e}, yardstick {yard:.3e}, w spans {w64.min().item():.4f} .. {w64.max().item():.4f}")
    assert w.dtype == torch.float32 and tuple(w.shape) == tuple(labels.shape) and w.is_contiguous()
    assert yard > 0 and err <= 4 * yard, (err, yard)
    assert w.min().item() >= floor and w.max().item() <= 1.0


def test_confidence_special_values(dev):
    """``w == 1`` where the sentinel applies; ``w`` at d^2 = 1 equals the formula - to 2e-7: the quotient, the exponential and
    the two final operations each round a value of at most 1 once, half a float32 ulp (6e-8) each; ``floor=1``: all ones."""
    import math
    from weaklysuperviseddl_amd import ops
    labels, _ = reference(4)
    batch = torch.cat([labels[:1], torch.ones(1, 37, 53, dtype=torch.int64), torch.zeros(1, 37, 53, dtype=torch.int64)]).to(dev)
    w = ops.boundary_confidence(batch, 3.0, 0.25)
    assert (w[1:] == 1).all() and (w[0] < 1).any()
    d_out, d_in = ops.edt(batch)
    at1 = w[(d_out + d_in) == 1]
    want = 0.25 + 0.75 * (1 - math.exp(-1 / 18.0))
    assert at1.numel() > 0 and (at1 == at1[0]).all() and abs(at1[0].item() - want) <= 2e-7, (at1[0].item(), want)
    ones = ops.boundary_confidence(batch, 3.0, 1.0)
    assert torch.equal(ones, torch.ones_like(ones))
    # out=: the map and both planes land in the caller's buffers
    bufs = {}
    w2 = ops.boundary_confidence(batch, 3.0, 0.25, out=bufs)
    assert w2 is bufs["weight"] and torch.equal(w2, w) and torch.equal(bufs["out"], d_out) and torch.equal(bufs["in"], d_in)
    ptr = w2.data_ptr()
    assert ops.boundary_confidence(batch, 3.0, 0.25, out=bufs).data_ptr() == ptr
    with pytest.raises(ValueError):
        ops.boundary_confidence(batch, 0.0)
    with pytest.raises(ValueError):
        ops.boundary_confidence(batch, 3.0, -0.1)


# ------------------------------------------------------------------------------------------------------ 6. the criterion
@pytest.mark.parametrize("weighted", (False, True))
def test_criterion_is_bit_identical_to_the_weighted_cross_entropy(dev, weighted):
    from weaklysuperviseddl_amd import ops, nn as wnn
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(2, 2, 33, 47, generator=g).to(dev)
    labels = (eo.make_labels(2, 33, 47, 61) == 1).long()
    kw = {}
    if weighted:
        labels[:, 5:9, 30:40] = 255
        kw = dict(weight=torch.tensor([0.7, 1.9]).to(dev), ignore_index=255, label_smoothing=0.1)
    labels = labels.to(dev)
    crit = wnn.BoundaryAwareCrossEntropyLoss(sigma=2.5, floor=0.2, **kw).to(dev)
    ref = wnn.CrossEntropyLoss(**kw).to(dev)
    ref.set_pixel_weight(ops.boundary_confidence(labels, 2.5, 0.2))
    za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    la, lb = crit(za, labels), ref(zb, labels)
    la.backward()
    lb.backward()
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0
    assert torch.equal(crit.pixel_weight, ref.pixel_weight) and crit.d2_out.dtype == torch.int32
    # the buffers keep their addresses from call to call and move with the shape
    ptrs = (crit.pixel_weight_ptr, crit.d2_out_ptr, crit.d2_in_ptr)
    crit(za.detach(), labels)
    assert ptrs == (crit.pixel_weight_ptr, crit.d2_out_ptr, crit.d2_in_ptr) == (crit.pixel_weight.data_ptr(), crit.d2_out.data_ptr(), crit.d2_in.data_ptr())
    crit(za.detach()[:, :, :20].contiguous(), labels[:, :20].contiguous())
    assert tuple(crit.pixel_weight.shape) == (2, 20, 47) and crit.pixel_weight_shape == "2x20x47"
    # floor = 1: the plain cross entropy with a weight of ones
    plain = wnn.CrossEntropyLoss(**kw).to(dev)
    plain.set_pixel_weight(torch.ones(2, 33, 47, device=dev))
    assert torch.equal(wnn.BoundaryAwareCrossEntropyLoss(floor=1.0, **kw).to(dev)(logits, labels), plain(logits, labels))


def test_plan_key_holds_the_options():
    from weaklysuperviseddl_amd import plan, nn as wnn
    base = plan.host_scalars(wnn.BoundaryAwareCrossEntropyLoss())
    assert base == plan.host_scalars(wnn.BoundaryAwareCrossEntropyLoss())
    for kw in (dict(sigma=2.0), dict(floor=0.1), dict(value=2), dict(ignore_index=255), dict(reduction="sum"), dict(label_smoothing=0.1)):
        assert plan.host_scalars(wnn.BoundaryAwareCrossEntropyLoss(**kw)) != base, kw
    with pytest.raises(ValueError):
        wnn.BoundaryAwareCrossEntropyLoss(sigma=-1.0)
    with pytest.raises(ValueError):
        wnn.BoundaryAwareCrossEntropyLoss(floor=2.0)


# ------------------------------------------------------------------------------------------------------ 7. planned step
def test_planned_step_replays_and_a_new_sigma_records_a_new_plan(dev):
    """Seven steps on the smallest configuration of tests/test_hip_plan.py (the reference's model, 4 x 64 x 64), two batches with
    different masks in turn: eager, eager, record (+ verification on a probe batch with the masks inverted), replay; then
    sigma changes: eager (a key seen once), record, replay.  Every loss and the final state equal the eager run's bit for
    bit; a run that keeps the old sigma - what a stale plan would compute - has another loss at step 5."""
    from weaklysuperviseddl_amd import plan, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(4, 3, 64, 64, generator=g).to(dev), (eo.make_labels(4, 64, 64, 70 + i) == 1).long().to(dev))
               for i in range(2)]
    assert not torch.equal(batches[0][1], batches[1][1])

    def run(planned, sigmas):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = build_segmentation_model().to(dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = wnn.BoundaryAwareCrossEntropyLoss(sigma=sigmas[0], floor=0.1)
            torch.manual_seed(1234)
            losses = []
            for i, sigma in enumerate(sigmas):
                crit.sigma = sigma
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
            torch.cuda.synchronize()
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st
        finally:
            plan.PLAN_STEP[0] = old

    changing = [3.0] * 4 + [1.0] * 3
    l0, s0, _ = run(False, changing)
    l1, s1, st = run(True, changing)
    stale, _, _ = run(False, [3.0] * 5)
    print(f"planned boundary-aware step: losses {l1}, records {st.records}, replays {st.replays}; step 5 with the old sigma {stale[4]}")
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.records == 2 and st.replays == 2, (st.records, st.replays)
    assert l0 == l1 and all(v == v for v in l0), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert stale[:4] == l0[:4] and stale[4] != l0[4]


# ------------------------------------------------------------------------------------------------------ 8. evaluation
def test_evaluate_boundary_iou_equals_the_oracle(dev):
    """A stub model whose logits come from a table keyed on the image's first value; two batches, the first image of each
    counts, one of them with a ground truth of another size (nearest resize of the prediction)."""
    from weaklysuperviseddl_amd.TraditionalModel import evaluate_boundary_iou

    preds = eo.make_labels(2, 37, 53, 81)
    preds = (preds == 1).long()

    class Stub(torch.nn.Module):
        def forward(self, x):
            p = preds[int(x[0, 0, 0, 0].item())].to(x.device)
            return {"out": torch.stack([1.0 - p.float(), p.float()])[None]}

    def image(i):
        return torch.full((2, 3, 37, 53), float(i))

    # Oxford-IIIT Pet trimaps: 1 = pet, 2 = background, 3 = border ("modular"); the notebook's loader hands them out as 0, 1, 2
    tri0 = torch.where(torch.roll(preds[0], (1, -2), (0, 1)) == 1, 1, 2)
    tri0[0:3, 0:9] = 3
    tri1 = torch.where(eo.make_labels(1, 50, 40, 82)[0] == 1, 1, 2)

    for binarize in ("notebook", "modular"):
        shift = 1 if binarize == "notebook" else 0
        loader = [(image(i), (torch.zeros(2), torch.stack([t - shift, t - shift]))) for i, t in enumerate((tri0, tri1))]
        counts = []
        for (img, (_l, tm)), p in zip(loader, preds):
            gt = tm[0].clone()
            if binarize == "notebook":
                gt[gt == 2] = 1
                gt = 1 - gt
            else:
                gt = (gt == 1).long()
            if p.shape != gt.shape:
                iy = torch.arange(gt.shape[0]) * p.shape[0] // gt.shape[0]
                ix = torch.arange(gt.shape[1]) * p.shape[1] // gt.shape[1]
                p = p[iy][:, ix]
            counts += eo.boundary_iou_counts(p[None], gt[None], eo.boundary_width(*gt.shape, 0.05))
        got = evaluate_boundary_iou(Stub(), loader, device=dev, binarize=binarize, ratio=0.05)
        assert isinstance(got, float) and got == eo.mean_iou(counts) and 0.0 < got < 1.0, (binarize, got, counts)
