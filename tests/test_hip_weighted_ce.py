"""The weighted cross entropy on the device: ``ops.cross_entropy`` with class weights, pixel weights, label smoothing and
the three reductions (wsdl_softmax_ce_ex_fwd_bwd) against torch CPU float64 / the float64 oracle, its edge cases, the
untouched default path, planned training steps and ``ops.class_weights_from_labels``."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from weighted_ce_oracle import weighted_ce  # noqa: E402

# Every test that takes the `dev` fixture MUST carry @gpu (see test_hip_small_ops.py)
gpu = pytest.mark.gpu

# the project's bound for this kernel (test_hip_small_ops.py, test_hip_ops.py::test_cross_entropy): relative max-norm error
REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def make_case(shape, seed, ignore_index=-100, scale=3.0):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g) * scale
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.2] = ignore_index
    w = torch.rand(C, generator=g) + 0.25
    p = torch.rand(B, H, W, generator=g) + 0.05
    up = torch.rand(B, H, W, generator=g) + 0.5
    return z, y, w, p, up


def run_device(dev, z, y, ignore_index=-100, weight=None, eps=0.0, reduction="mean", pw=None, upstream=None):
    from weaklysuperviseddl_amd import ops
    zd = z.to(dev).requires_grad_(True)
    loss = ops.cross_entropy(zd, y.to(dev), ignore_index, weight=None if weight is None else weight.to(dev),
                             label_smoothing=eps, reduction=reduction, pixel_weight=None if pw is None else pw.to(dev))
    if upstream is None:
        upstream = torch.ones(loss.shape)
    loss.backward(upstream.to(dev))
    return loss.detach().cpu(), zd.grad.cpu()


OPTIONS = list(itertools.product((False, True), (0.0, 0.1), (False, True), ("mean", "sum", "none")))


# C = 2, 3: the unrolled register forms; 1, 8: the predicated 8-register form (8 is its limit); 9, 21, 37: the form that
# re-reads memory.  (2,C,5,7): odd H*W and a batch stride; (1,C,16,16): exactly one block.  The bound is not widened for
# C >= 21 with smoothing: the same formula by torch on the CPU in float32 is within 1.1e-6 of float64 on these very cases.
@gpu
@pytest.mark.parametrize("C", (1, 2, 3, 8, 9, 21, 37))
@pytest.mark.parametrize("BHW", ((2, 5, 7), (1, 16, 16)))
def test_parity_grid_against_float64(dev, BHW, C):
    shape = (BHW[0], C, BHW[1], BHW[2])
    z, y, w, p, up = make_case(shape, 1000 + 10 * C + BHW[0])
    worst = 0.0
    for weighted, eps, pixel, reduction in OPTIONS:
        upstream = up if reduction == "none" else torch.tensor(0.7)
        weight, pw = (w if weighted else None), (p if pixel else None)
        loss, grad = run_device(dev, z, y, -100, weight, eps, reduction, pw, upstream)
        if pixel:
            ref_loss, ref_grad = weighted_ce(z, y, -100, weight, eps, reduction, pixel_weight=pw, upstream=upstream)
        else:       # torch CPU float64
            zt = z.double().requires_grad_(True)
            ref_loss = F.cross_entropy(zt, y, weight=None if weight is None else weight.double(), reduction=reduction,
                                       label_smoothing=eps)
            ref_loss.backward(upstream.double())
            ref_loss, ref_grad = ref_loss.detach(), zt.grad
        what = (shape, weighted, eps, pixel, reduction)
        assert loss.shape == ref_loss.shape and loss.dtype == torch.float32, what
        el = rel_err(loss, ref_loss)
        eg = rel_err(grad, ref_grad) if C > 1 else float((grad.double() - ref_grad).abs().max())   # C = 1: the gradient is 0
        worst = max(worst, el, eg)
        assert el <= REL and eg <= REL, (what, el, eg)
    print(f"weighted CE parity {shape}: worst rel err {worst:.3e} (bound {REL:.0e})")


@gpu
def test_grid_stride_loop_with_every_option_on(dev):
    """525 312 pixels: more than the 2048 blocks x 256 threads of one pass of the grid."""
    shape = (2, 3, 513, 512)
    z, y, w, p, up = make_case(shape, 5)
    for reduction, upstream in (("mean", torch.tensor(0.7)), ("none", up)):
        loss, grad = run_device(dev, z, y, -100, w, 0.1, reduction, p, upstream)
        ref_loss, ref_grad = weighted_ce(z, y, -100, w, 0.1, reduction, pixel_weight=p, upstream=upstream)
        assert rel_err(loss, ref_loss) <= REL and rel_err(grad, ref_grad) <= REL, reduction


@gpu
def test_edge_cases_follow_torch(dev):
    shape = (2, 3, 5, 7)
    z, y, w, p, up = make_case(shape, 11)
    # every label ignored: mean NaN, sum 0, a map of zeros; zero gradient
    yi = torch.full_like(y, -100)
    for kw in ({}, {"weight": w, "eps": 0.1, "pw": p}):
        loss, grad = run_device(dev, z, yi, reduction="mean", **kw)
        assert torch.isnan(loss) and not grad[~torch.isnan(grad)].any()
        loss, grad = run_device(dev, z, yi, reduction="sum", **kw)
        assert loss.item() == 0.0 and not grad.any()
        loss, grad = run_device(dev, z, yi, reduction="none", **kw)
        assert not loss.any() and not grad.any()
    assert torch.isnan(F.cross_entropy(z, yi)) and F.cross_entropy(z, yi, reduction="sum").item() == 0.0
    # a present class with weight 0: as torch
    w0 = w.clone()
    w0[1] = 0.0
    for eps, reduction in itertools.product((0.0, 0.1), ("mean", "sum", "none")):
        loss, grad = run_device(dev, z, y, weight=w0, eps=eps, reduction=reduction)
        zt = z.double().requires_grad_(True)
        ref = F.cross_entropy(zt, y, weight=w0.double(), reduction=reduction, label_smoothing=eps)
        ref.backward(torch.ones_like(ref))
        assert rel_err(loss, ref) <= REL and rel_err(grad, zt.grad) <= REL, (eps, reduction)
    # every present class with weight 0: 0/0
    y01 = y.clamp(-100, 1)
    wz = torch.tensor([0.0, 0.0, 1.5])
    loss, _ = run_device(dev, z, y01, weight=wz)
    assert torch.isnan(loss) and torch.isnan(F.cross_entropy(z, y01, weight=wz))
    # one label that is no class: NaN for mean and sum, NaN at that pixel only for none
    yb = y.clone()
    yb[1, 2, 3] = 3
    for kw in ({}, {"weight": w}, {"eps": 0.1}, {"pw": p}):
        for reduction in ("mean", "sum"):
            loss, _ = run_device(dev, z, yb, reduction=reduction, **kw)
            assert torch.isnan(loss), (kw, reduction)
        loss, _ = run_device(dev, z, yb, reduction="none", **kw)
        nan = torch.isnan(loss)
        assert nan[1, 2, 3] and nan.sum() == 1, kw
    # large logits stay finite
    for kw in ({}, {"weight": w, "eps": 0.1, "pw": p}):
        loss, grad = run_device(dev, z * 1e4, y, **kw)
        ref_loss, ref_grad = weighted_ce(z * 1e4, y, -100, kw.get("weight"), kw.get("eps", 0.0), "mean", pixel_weight=kw.get("pw"))
        assert torch.isfinite(loss) and torch.isfinite(grad).all()
        assert rel_err(loss, ref_loss) <= REL and rel_err(grad, ref_grad) <= REL
    # eps = 1: the target only counts through the denominator
    for weight, reduction in itertools.product((None, w), ("mean", "sum", "none")):
        loss, grad = run_device(dev, z, y, weight=weight, eps=1.0, reduction=reduction)
        zt = z.double().requires_grad_(True)
        ref = F.cross_entropy(zt, y, weight=None if weight is None else weight.double(), reduction=reduction, label_smoothing=1.0)
        ref.backward(torch.ones_like(ref))
        assert rel_err(loss, ref) <= REL and rel_err(grad, zt.grad) <= REL, (weight is not None, reduction)


@gpu
@pytest.mark.parametrize("C", (2, 8, 21))
def test_metamorphic_relations(dev, C):
    z, y, w, p, up = make_case((2, C, 9, 13), 40 + C)
    drop = torch.rand(2, 9, 13, generator=torch.Generator().manual_seed(C)) < 0.2
    for eps, reduction in itertools.product((0.0, 0.1), ("mean", "sum", "none")):
        upstream = up if reduction == "none" else torch.tensor(0.7)
        # a zero pixel weight IS an ignored pixel: the same bits
        a = run_device(dev, z, y, -100, w, eps, reduction, torch.where(drop, torch.zeros_like(p), p), upstream)
        b = run_device(dev, z, torch.where(drop, torch.full_like(y, -100), y), -100, w, eps, reduction,
                       torch.where(drop, torch.ones_like(p), p), upstream)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (eps, reduction)
        # two identical calls: the same bits
        c = run_device(dev, z, y, -100, w, eps, reduction, p, upstream)
        d = run_device(dev, z, y, -100, w, eps, reduction, p, upstream)
        assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]), (eps, reduction)
    # weights of one are the default call
    one = run_device(dev, z, y, weight=torch.ones(C), pw=torch.ones(2, 9, 13), upstream=torch.tensor(0.7))
    plain = run_device(dev, z, y, upstream=torch.tensor(0.7))
    assert rel_err(one[0], plain[0]) <= 1e-6 and rel_err(one[1], plain[1]) <= 1e-6


class _Recorder:
    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._real, name)


@gpu
def test_default_call_goes_through_the_old_entry_point(dev, monkeypatch):
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd._lib import lib
    z, y, w, _, _ = make_case((2, 3, 9, 13), 8)
    zd, yd = z.to(dev), y.to(dev)
    names = []
    monkeypatch.setattr(ops, "lib", lambda: _Recorder(lib(), names))
    a = ops.cross_entropy(zd.clone().requires_grad_(True), yd)
    b = ops.cross_entropy(zd.clone().requires_grad_(True), yd, -100)
    assert "wsdl_softmax_ce_fwd_bwd" in names and "wsdl_softmax_ce_ex_fwd_bwd" not in names
    del names[:]
    ops.cross_entropy(zd, yd, weight=w.to(dev))
    assert "wsdl_softmax_ce_ex_fwd_bwd" in names and "wsdl_softmax_ce_fwd_bwd" not in names
    monkeypatch.undo()
    # the old symbol and the new one without options: the same bits, loss and unnormalised gradient
    out = []
    for ex in (False, True):
        loss = torch.empty((), device=dev)
        dl, inv = torch.empty_like(zd), torch.empty(1, device=dev)
        ws = ops.workspace(lib().wsdl_reduce_workspace(), dev)
        head = (zd.data_ptr(), yd.data_ptr(), loss.data_ptr(), dl.data_ptr(), inv.data_ptr(), 2, 3, 9, 13, 1.0, -100)
        tail = (ws.data_ptr(), ws.numel(), ops._stream())
        if ex:
            ops.check(lib().wsdl_softmax_ce_ex_fwd_bwd(*head, None, None, 0.0, 0, *tail))
        else:
            ops.check(lib().wsdl_softmax_ce_fwd_bwd(*head, *tail))
        out.append((loss.cpu(), dl.cpu(), inv.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*out))
    assert torch.equal(a.detach().cpu(), out[0][0]) and torch.equal(b.detach().cpu(), out[0][0])
    # options the ABI refuses
    for eps, reduction in ((1.5, 0), (-0.1, 0), (0.0, 3), (0.0, -1)):
        assert lib().wsdl_softmax_ce_ex_fwd_bwd(*head, None, None, eps, reduction, *tail) != 0


def _planned_and_eager(dev, make_criterion, before_step=None):
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.FullySupervisedModel.SupervisedModel import initialize_model
    from weaklysuperviseddl_amd.TraditionalModel import train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    gen = torch.Generator().manual_seed(2)
    batches = [((torch.rand(4, 3, 64, 64, generator=gen)).to(dev), (torch.rand(4, 64, 64, generator=gen) > 0.5).long().to(dev))
               for _ in range(2)]

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = initialize_model(2, device=dev).train()
            opt = make_optimizer(model, lr=1e-4)
            crit = make_criterion()
            torch.manual_seed(1234)
            losses = []
            for i in range(4):
                if before_step is not None:
                    before_step(crit, i)
                losses.append(float(train_step(model, opt, *batches[i % 2], criterion=crit)))
            torch.cuda.synchronize()
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            state = [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()]
            return losses, state, st
        finally:
            plan.PLAN_STEP[0] = old

    l0, s0, _ = run(False)
    l1, s1, st = run(True)
    assert st is not None and st.disabled is None, getattr(st, "disabled", "no planned step")
    assert st.replays >= 1, (st.records, st.replays)
    assert l0 == l1 and all(np.isfinite(l0))
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    return l0


@gpu
def test_planned_step_with_class_weights_is_bit_identical_to_eager(dev):
    weight = torch.tensor([0.3, 1.7], device=dev)
    _planned_and_eager(dev, lambda: torch.nn.CrossEntropyLoss(weight=weight))


@gpu
def test_planned_step_reads_pixel_weights_refilled_before_every_step(dev):
    """The maps differ from step to step: a replay that read the values of the recorded step could not equal the eager run."""
    import weaklysuperviseddl_amd.nn as wnn
    gen = torch.Generator().manual_seed(9)
    maps = [torch.rand(4, 64, 64, generator=gen).to(dev) for _ in range(4)]
    _planned_and_eager(dev, lambda: wnn.CrossEntropyLoss(label_smoothing=0.1), lambda crit, i: crit.set_pixel_weight(maps[i]))


@gpu
def test_class_weights_from_labels(dev):
    from weaklysuperviseddl_amd import ops
    C = 5
    g = torch.Generator().manual_seed(4)
    y = torch.randint(0, 4, (3, 9, 13), generator=g)
    y[y == 2] = 3                                   # class 2 (and 4) absent
    y[torch.rand(3, 9, 13, generator=g) < 0.2] = 255
    n = np.array([(y.numpy() == c).sum() for c in range(C)], dtype=np.float64)
    safe = np.where(n > 0, n, 1.0)
    inverse = np.where(n > 0, n.sum() / (C * safe), 0.0)
    median = np.where(n > 0, np.median(n) / safe, 0.0)
    for ignore in (255, None):                      # 255 is no class: left out with or without ignore=
        wi = ops.class_weights_from_labels(y.to(dev), C, ignore)
        wm = ops.class_weights_from_labels(y.to(dev), C, ignore, mode="median")
        assert wi.is_cuda and wi.dtype == torch.float32 and tuple(wi.shape) == (C,)
        np.testing.assert_allclose(wi.cpu().numpy(), inverse, rtol=1e-6)
        np.testing.assert_allclose(wm.cpu().numpy(), median, rtol=1e-6)
        assert wi[2] == 0 and wi[4] == 0
    # an ignored label that is a class counts as absent
    n3 = n.copy()
    n3[3] = 0
    w3 = ops.class_weights_from_labels(y.to(dev), C, 3)
    np.testing.assert_allclose(w3.cpu().numpy(), np.where(n3 > 0, n3.sum() / (C * np.where(n3 > 0, n3, 1.0)), 0.0), rtol=1e-6)
    # the weights feed the loss as they are
    z = torch.randn(3, C, 9, 13, generator=g)
    loss = ops.cross_entropy(z.to(dev), y.to(dev), 255, weight=wi)
    ref = F.cross_entropy(z.double(), y, weight=torch.from_numpy(inverse), ignore_index=255)
    assert rel_err(loss, ref) <= REL
