"""Device-wide component labelling, seeded region growing, the balanced seed weights, ``SeededRegionGrowingLoss`` and a planned
training step with it (csrc/components_grid.hip) against the numpy + scipy oracle of tests/srg_oracle.py.  Everything integer is
EQUAL, never close.  The criterion's loss and gradient follow the parity rule of tests/test_hip_overlap_loss.py: the same oracle
in float32 on the CPU against its float64 run is the yardstick, the device may be off the float64 value by at most
``max(4 x that, 2^-23 x |float64 value|)``; the worst ratio is reported with ``report_line``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srg_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

IGN = so.IGNORE
FLOOR = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def maps():
    return so.structured_maps()


def T(a):
    """A torch copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def shape_name(i):
    return "x".join(str(v) for v in so.SHAPES[i])


def device_grow(dev, scores, seeds, thresh, **kw):
    from weaklysuperviseddl_amd import ops
    thresh = thresh.tolist() if isinstance(thresh, np.ndarray) else thresh
    out = {}
    present = kw.pop("present", None)
    if present is not None:
        present = T(np.asarray(present).astype(np.uint8)).to(dev)
    grown, counts = ops.seeded_region_growing(T(scores).to(dev), T(seeds).to(dev), thresh, present=present,
                                              out=out, **kw)
    assert int(out["error"].item()) == 0
    return grown.cpu().numpy(), counts.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. label_components
@pytest.mark.parametrize("name", sorted(so.structured_maps()))
def test_label_components_on_structured_maps(dev, name):
    from weaklysuperviseddl_amd import ops
    m = maps()[name]
    labels = T(m).to(dev)
    before = labels.clone()
    for conn in (8, 4):
        for bg in (None, 0):
            want, want_area = so.components(m, bg, conn, want_area=True)
            out = {}
            comp, area = ops.label_components(labels, background=bg, connectivity=conn, want_area=True, out=out)
            assert comp.dtype == torch.int32 and area.dtype == torch.int32 and out["comp"] is comp and out["area"] is area
            assert int(out["error"].item()) == 0
            comp_h, area_h = comp.cpu().numpy(), area.cpu().numpy()
            assert np.array_equal(comp_h, want), (name, conn, bg, int((comp_h != want).sum()))
            for b in range(m.shape[0]):                                     # the areas against np.bincount of the labels themselves
                valid = comp_h[b] >= 0
                n = np.bincount(comp_h[b][valid], minlength=1)
                assert np.array_equal(area_h[b][valid], n[comp_h[b][valid]]) and not area_h[b][~valid].any(), (name, conn, bg, b)
            assert np.array_equal(area_h, want_area)
            ptrs = (comp.data_ptr(), area.data_ptr())
            comp2 = ops.label_components(labels, background=bg, connectivity=conn, out=out)     # the caller's buffer, no areas
            assert comp2.data_ptr() == ptrs[0] and out["area"].data_ptr() == ptrs[1] and np.array_equal(comp2.cpu().numpy(), want)
    assert torch.equal(labels, before)


def test_label_components_takes_masks_and_refuses_what_the_library_refuses(dev):
    from weaklysuperviseddl_amd import ops, _lib
    m = maps()["random_2"]
    want = so.components(m, 0, 8)
    for t in (T(m.astype(np.uint8)), T(m.astype(bool))):
        assert np.array_equal(ops.label_components(t.to(dev), background=0).cpu().numpy(), want)
    lib = _lib.lib()
    assert lib.wsdl_label_components_workspace(1, 65, 130) >= 4
    for geom in ((0, 4, 4), (1, -1, 4), (2, 1 << 15, 1 << 15), (1, 1 << 16, 1 << 15)):
        assert lib.wsdl_label_components_workspace(*geom) == 0
        assert lib.wsdl_seeded_region_growing_workspace(geom[0], 2, geom[1], geom[2]) == 0
    assert lib.wsdl_label_components_workspace(1, 1, 2 ** 31 - 1) >= 4
    lab = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)
    comp = torch.empty(1, 4, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(64, dtype=torch.uint8, device=dev)
    args = lambda conn, B: (lab.data_ptr(), B, 4, 4, conn, 0, 0, comp.data_ptr(), None, ws.data_ptr(), ws.numel(), None)   # noqa: E731
    assert lib.wsdl_label_components(*args(6, 1)) != 0 and b"connectivity" in lib.wsdl_last_error()
    assert lib.wsdl_label_components(*args(8, 0)) != 0


# ------------------------------------------------------------------------------------------------ 2. region growing
@pytest.mark.parametrize("i", range(len(so.SHAPES)))
def test_region_growing_equals_the_oracle(dev, i):
    from weaklysuperviseddl_amd import ops
    from conftest import report_line
    scores, seeds, thresh, want, want_counts, stats = so.case(i)
    sc, se = T(scores).to(dev), T(seeds).to(dev)
    sc0, se0 = sc.clone(), se.clone()
    out = {}
    grown, counts = ops.seeded_region_growing(sc, se, thresh.tolist(), ignore_index=IGN, out=out)
    assert grown.dtype == torch.int64 and counts.dtype == torch.int64 and int(out["error"].item()) == 0
    g, c = grown.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(g, want), (so.SHAPES[i], int((g != want).sum()))
    assert np.array_equal(c, want_counts)
    # the out= buffers are reused, a second call is bit-identical, the inputs are never written
    ptrs = (grown.data_ptr(), counts.data_ptr())
    g2, c2 = ops.seeded_region_growing(sc, se, thresh.tolist(), ignore_index=IGN, out=out)
    assert (g2.data_ptr(), c2.data_ptr()) == ptrs and np.array_equal(g2.cpu().numpy(), g) and np.array_equal(c2.cpu().numpy(), c)
    assert torch.equal(sc, sc0) and torch.equal(se, se0)
    # the thresholds in a device buffer
    g3, c3 = ops.seeded_region_growing(sc, se, T(thresh).to(dev), ignore_index=IGN)
    assert np.array_equal(g3.cpu().numpy(), g) and np.array_equal(c3.cpu().numpy(), c)
    report_line(f"seeded region growing {shape_name(i)}: {stats['grown']} of {stats['components']} components grow, "
                f"{int((g != IGN).sum())} of {g.size} pixels labelled: equal")


def test_region_growing_edge_cases(dev):
    scores, seeds, thresh, want, _, _ = so.case(4)                           # 3x3x37x53
    B, C, H, W = scores.shape
    # no seed: everything is ignore_index; another ignore_index
    none = np.full(seeds.shape, -7, dtype=np.int64)
    g, c = device_grow(dev, scores, none, thresh, ignore_index=-100)
    assert (g == -100).all() and not c.any()
    # every pixel seeded: the seeds come back
    full = np.random.default_rng(3).integers(0, C, seeds.shape)
    g, c = device_grow(dev, scores, full, thresh)
    assert np.array_equal(g, full) and np.array_equal(c, np.stack([np.bincount(full[b].ravel(), minlength=C) for b in range(B)]))
    # the present mask, different per image
    pres = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=bool)
    wg, wc = so.grow(scores, seeds, thresh, present=pres)
    assert not np.array_equal(wg, want)
    g, c = device_grow(dev, scores, seeds, thresh, present=pres)
    assert np.array_equal(g, wg) and np.array_equal(c, wc)
    # NaN scores, a tie of two scores, a (bg, fg) pair
    s2 = scores.copy()
    s2[:, 0, ::5, ::3] = np.nan
    s2[:, 1, 1::4] = s2[:, 2, 1::4]
    pair = (0.6, 0.45)
    wg, wc = so.grow(s2, seeds, [pair[0]] + [pair[1]] * (C - 1))
    g, c = device_grow(dev, s2, seeds, pair)
    assert np.array_equal(g, wg) and np.array_equal(c, wc)


def test_more_classes_than_travel_by_value(dev):
    B, C, H, W = 1, 40, 9, 70
    scores = so.make_scores(B, C, H, W, 5)
    seeds = so.make_seeds(scores, 6)
    thresh = np.linspace(0.05, 0.3, C).astype(np.float32)
    wg, wc = so.grow(scores, seeds, thresh)
    assert ((wg != IGN) & (seeds == IGN)).any()
    g, c = device_grow(dev, scores, seeds, thresh)
    assert np.array_equal(g, wg) and np.array_equal(c, wc)


# ------------------------------------------------------------------------------------------------ 3. weights
@pytest.mark.parametrize("i", (3, 4, 5))
def test_balanced_seed_weights(dev, i):
    from weaklysuperviseddl_amd import ops
    _, _, _, grown, counts, _ = so.case(i)
    B, C = counts.shape
    g, c = T(grown).to(dev), T(counts).to(dev)
    buf = torch.empty(grown.shape, dtype=torch.float32, device=dev)
    for balance in ("fg_bg", "class", "none"):
        w = ops.balanced_seed_weights(g, c, balance=balance, out=buf)
        assert w is buf
        want = so.weights(grown, counts, balance).astype(np.float32)        # np.float32(1.0 / (B * n)): the double rounded once
        assert np.array_equal(w.cpu().numpy(), want), (so.SHAPES[i], balance)
        assert (want[grown == IGN] == 0).all() and (want[grown != IGN] > 0).all()
    # a group the counts call empty: 0, not a division by zero
    c0 = counts.copy()
    c0[:, 1:] = 0
    w = ops.balanced_seed_weights(g, T(c0).to(dev)).cpu().numpy()
    assert np.isfinite(w).all() and not w[grown > 0].any() and np.array_equal(w, so.weights(grown, c0, "fg_bg").astype(np.float32))


# ------------------------------------------------------------------------------------------------ 4. the criterion
def logits_of(i):
    scores = so.case(i)[0]
    return np.log(np.maximum(scores, 1e-30)).astype(np.float32) + np.float32(0.25)


@pytest.mark.parametrize("balance", ("fg_bg", "class", "none"))
def test_criterion_equals_cross_entropy_on_its_published_buffers(dev, balance):
    from weaklysuperviseddl_amd import ops, nn as wnn
    _, seeds, thresh, _, _, _ = so.case(4)
    logits, se = T(logits_of(4)).to(dev), T(seeds).to(dev)
    crit = wnn.SeededRegionGrowingLoss(thresh=thresh.tolist(), balance=balance, ignore_index=IGN).to(dev)
    za, zb = logits.clone().requires_grad_(), logits.clone().requires_grad_()
    la = crit(za, se)
    la.backward()
    lb = ops.cross_entropy(zb, crit.grown, IGN, reduction="mean" if balance == "none" else "sum", pixel_weight=crit.pixel_weight)
    lb.backward()
    assert torch.isfinite(la) and la.item() > 0 and torch.equal(la, lb) and torch.equal(za.grad, zb.grad) and za.grad.abs().sum() > 0
    assert crit.grown_ptr == crit.grown.data_ptr() and crit.thresh_ptr == crit.thresh.data_ptr() and crit.thresh_shape == "3"
    assert crit.pixel_weight_ptr == crit.pixel_weight.data_ptr() and crit.counts_ptr == crit.counts.data_ptr()
    assert crit.pixel_weight_shape == "3x37x53"
    # the buffers stay where they are on the next call and through set_thresh, which changes what grows
    ptrs = (crit.grown_ptr, crit.counts_ptr, crit.pixel_weight_ptr, crit.thresh_ptr)
    labelled = int((crit.grown != IGN).sum())
    crit.set_thresh(0.95)
    crit(logits, se)
    assert ptrs == (crit.grown_ptr, crit.counts_ptr, crit.pixel_weight_ptr, crit.thresh_ptr)
    assert crit.thresh.tolist() == [np.float32(0.95)] * 3 and int((crit.grown != IGN).sum()) < labelled


@pytest.mark.parametrize("i", (3, 4, 6))
def test_criterion_loss_and_gradient_against_float64(dev, i):
    from weaklysuperviseddl_amd import ops, nn as wnn
    from conftest import report_line
    _, seeds, thresh, _, _, _ = so.case(i)
    logits = logits_of(i)
    B = logits.shape[0]
    zd, se = T(logits).to(dev), T(seeds).to(dev)
    probs = ops.softmax_channels(zd).cpu().numpy()
    worst = 0.0
    for balance in ("fg_bg", "class", "none"):
        crit = wnn.SeededRegionGrowingLoss(thresh=thresh.tolist(), balance=balance, ignore_index=IGN).to(dev)
        z = zd.clone().requires_grad_()
        loss = crit(z, se)
        loss.backward()
        stats = {}
        grown, counts = so.grow(probs, seeds, thresh, stats=stats)
        assert 0 < stats["grown"] and np.array_equal(crit.grown.cpu().numpy(), grown) and np.array_equal(crit.counts.cpu().numpy(), counts)
        w = so.weights(grown, counts, balance).astype(np.float32)
        assert np.array_equal(crit.pixel_weight.cpu().numpy(), w)
        l64, g64 = so.seeding_loss(logits, grown, w, balance, torch.float64)
        l32, g32 = so.seeding_loss(logits, grown, w, balance, torch.float32)
        for what, got, w64, w32 in (("loss", loss.detach().cpu(), l64, l32), ("gradient", z.grad.cpu(), g64, g32)):
            err = (got.double() - w64).abs().max().item()
            yard = (w32.double() - w64).abs().max().item()
            bound = max(4.0 * yard, FLOOR * float(w64.abs().max()))
            print(f"srg {shape_name(i)} {balance} {what}: device error {err:.3e}, float32 oracle {yard:.3e}, bound {bound:.3e}")
            assert torch.isfinite(got).all() and err <= bound, (what, balance, err, yard, bound)
            worst = max(worst, err / bound)
        assert g64.abs().sum() > 0 and B >= 1
    report_line(f"seeded region growing loss {shape_name(i)}: worst |device - float64| / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 5. launch plan
def test_planned_step_replays_through_set_thresh_and_records_anew_for_another_balance(dev):
    """The pattern of the plan test in tests/test_hip_overlap_loss.py: ten steps on the reference's model at 4 x 64 x 64, two
    batches with different seeds in turn: eager, eager, record (+ verification on a probe batch), replay; then ``set_thresh`` -
    the SAME plan replays three more times; then ``balance`` changes: eager (a key seen once), record, replay.  Every loss and
    the final state equal the eager run's bit for bit; a run that keeps the old thresholds - what a plan with frozen thresholds
    would compute - has another loss at step 5.  Unseeded pixels are -100: ``train_step`` clamps its masks to at most 1."""
    from weaklysuperviseddl_amd import plan, nn as wnn
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    g = torch.Generator().manual_seed(2)

    def seeds():
        s = torch.randint(0, 2, (4, 64, 64), generator=g)
        return torch.where(torch.rand(4, 64, 64, generator=g) < 0.05, s, torch.full_like(s, -100))

    batches = [(torch.randn(4, 3, 64, 64, generator=g).to(dev), seeds().to(dev)) for _ in range(2)]
    assert not torch.equal(batches[0][1], batches[1][1])

    def run(planned, schedule):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = build_segmentation_model().to(dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = wnn.SeededRegionGrowingLoss(thresh=schedule[0][0], balance=schedule[0][1]).to(dev)
            torch.manual_seed(1234)
            losses, plans, labelled = [], [], []
            st = None
            for i, (thresh, balance) in enumerate(schedule):
                crit.set_thresh(thresh)
                crit.balance = balance
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
                labelled.append(int(crit.counts.sum()))
                st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
                plans.append(None if st is None else (id(st), st.records, st.replays))
            torch.cuda.synchronize()
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st, plans, labelled
        finally:
            plan.PLAN_STEP[0] = old

    lo, hi = (0.5, 0.5), (0.56, 0.53)
    schedule = [(lo, "fg_bg")] * 4 + [(hi, "fg_bg")] * 3 + [(hi, "class")] * 3
    l0, s0, _, _, n0 = run(False, schedule)
    l1, s1, st, plans, n1 = run(True, schedule)
    stale, _, _, _, _ = run(False, [(lo, "fg_bg")] * 5)
    print(f"planned SRG step: losses {l1}, labelled pixels {n1}, records {st.records}, replays {st.replays}; step 5 with the old "
          f"thresholds {stale[4]}")
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert plans[3][1:] == (1, 1) and plans[6][1:] == (1, 4), plans      # after set_thresh: the same plan, no new recording
    assert len({p[0] for p in plans if p is not None}) == 1
    assert st.records == 2 and st.replays == 5, (st.records, st.replays)  # another balance: a new plan
    assert l0 == l1 and all(v == v and v > 0 for v in l0), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert all(n > 4 * 64 * 64 * 0.05 * 1.5 for n in n0[:2]), n0         # regions did grow beyond the 5 % of seeds
    assert stale[:4] == l0[:4] and stale[4] != l0[4]
