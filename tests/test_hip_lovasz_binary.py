"""The binary half of the reference's Lovasz file on the device (csrc/lovasz_seg.hip through ops and the drop-in module
TraditionalModel/LossFunctions/Lovasz_Softmax_Loss.py): against the vectors of the reference's own function bodies
(tests/golden/lovasz_binary.npz) and, at full size, against the fp32 oracle (tests/lovasz_binary_oracle.py) - never a float64
one: the reference's fp32 Jaccard terms are what parity means (see the oracle's header)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_binary_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from weaklysuperviseddl_amd.TraditionalModel.LossFunctions import Lovasz_Softmax_Loss
    return Lovasz_Softmax_Loss


def cases(g, fn):
    return [m for m in json.loads(str(g["meta"])) if m["fn"] == fn]


def check_loss_and_grad(loss, grad, g, n, void=None):
    """The tolerances of test_lovasz_softmax_vs_golden_and_oracle."""
    ref_loss, ref = float(g[n + "_loss"]), T(g[n + "_grad"])
    d_loss = abs(loss.item() - ref_loss)
    d_grad = (grad.cpu() - ref).abs().max().item()
    print(f"{n}: loss {loss.item():.9g} ref {ref_loss:.9g} |d| {d_loss:.3e}; grad max|d| {d_grad:.3e} of max|ref| {ref.abs().max().item():.3e}")
    assert d_loss <= 1e-5 * max(1.0, abs(ref_loss)), (n, loss.item(), ref_loss)
    assert d_grad <= 1e-5 * ref.abs().max().item() + 1e-9, (n, d_grad)
    if void is not None:
        assert void.any() and (grad.cpu()[void] == 0).all(), n


def test_hinge_vs_reference_vectors(dev, golden, L):
    g = golden("lovasz_binary")
    for m in cases(g, "lovasz_hinge"):
        n = m["case"]
        x = T(g[n + "_logits"]).to(dev).requires_grad_()
        lab = T(g[n + "_labels"])
        loss = L.lovasz_hinge(x, lab.to(dev), m["per_image"], m["ignore"])
        loss.backward()
        check_loss_and_grad(loss, x.grad, g, n, None if m["ignore"] is None else lab == m["ignore"])
    # the flat form: B = 1, H = 1, W = P of the whole-batch case without ignore
    m = [m for m in cases(g, "lovasz_hinge") if not m["per_image"] and m["ignore"] is None][0]
    x = T(g[m["case"] + "_logits"]).reshape(-1).to(dev).requires_grad_()
    loss = L.lovasz_hinge_flat(x, T(g[m["case"] + "_labels"]).reshape(-1).to(dev))
    loss.backward()
    check_loss_and_grad(loss, x.grad.reshape(g[m["case"] + "_grad"].shape), g, m["case"])
    # every pixel void: 0, zero gradient
    x = torch.randn(2, 6, 7, device=dev, requires_grad=True)
    for per_image in (True, False):
        x.grad = None
        loss = L.lovasz_hinge(x, torch.full((2, 6, 7), 255, device=dev), per_image, 255)
        loss.backward()
        assert loss.item() == 0.0 and (x.grad == 0).all()


def test_softmax_class_lists_vs_reference_vectors(dev, golden, L):
    from weaklysuperviseddl_amd import ops
    g = golden("lovasz_binary")
    for m in cases(g, "lovasz_softmax"):
        n = m["case"]
        p = T(g[n + "_probas"]).to(dev).requires_grad_()
        lab = T(g[n + "_labels"])
        loss = L.lovasz_softmax(p, lab.to(dev), m["classes"], m["per_image"], m["ignore"])
        loss.backward()
        void = None
        if m["ignore"] is not None:
            void = (lab == m["ignore"]) if p.dim() == 3 else (lab == m["ignore"]).unsqueeze(1).expand(p.shape)
        check_loss_and_grad(loss, p.grad, g, n, void)
    # the flat form of the [0, 2] whole-batch case
    m = [m for m in cases(g, "lovasz_softmax") if m["classes"] == [0, 2] and not m["per_image"]][0]
    p4 = T(g[m["case"] + "_probas"])
    flat = p4.permute(0, 2, 3, 1).reshape(-1, p4.shape[1]).to(dev).requires_grad_()
    loss = L.lovasz_softmax_flat(flat, T(g[m["case"] + "_labels"]).reshape(-1).to(dev), [0, 2])
    loss.backward()
    back = flat.grad.reshape(p4.shape[0], p4.shape[2], p4.shape[3], p4.shape[1]).permute(0, 3, 1, 2)
    check_loss_and_grad(loss, back, g, m["case"])
    # one sigmoid map takes one class; a class listed twice is two equal terms: the same mean, the same gradient, same bits
    with pytest.raises(ValueError):
        L.lovasz_softmax(torch.rand(2, 4, 5, device=dev), torch.zeros(2, 4, 5, dtype=torch.long, device=dev), [0, 1])
    p1, p2 = T(g["softmax0_probas"]).to(dev).requires_grad_(), T(g["softmax0_probas"]).to(dev).requires_grad_()
    lab = T(g["softmax0_labels"]).to(dev)
    l1, l2 = ops.lovasz_softmax(p1, lab, [1]), ops.lovasz_softmax(p2, lab, [1, 1])
    l1.backward(), l2.backward()
    assert l1.item() == l2.item() and torch.equal(p1.grad, p2.grad)
    # outside what the reference defines: an all-void image is a zero term that counts; one valid pixel is computed
    lab = T(g["softmax1_labels"]).clone()
    lab[1] = 255
    p = T(g["softmax1_probas"]).requires_grad_()
    want = O.lovasz_softmax(p, lab, [0, 2], True, 255)
    want.backward()
    pd = T(g["softmax1_probas"]).to(dev).requires_grad_()
    got = ops.lovasz_softmax(pd, lab.to(dev), [0, 2], True, 255)
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    assert (pd.grad.cpu() - p.grad).abs().max().item() <= 1e-5 * p.grad.abs().max().item() + 1e-9 and (pd.grad[1] == 0).all()
    lab = torch.full((1, 4, 5), 255)
    lab[0, 2, 3] = 1
    x = torch.full((1, 4, 5), -0.5, device=dev, requires_grad=True)
    loss = ops.lovasz_hinge(x, lab.to(dev), True, 255)                    # e = 1.5, J_0 = 1
    loss.backward()
    assert loss.item() == 1.5 and x.grad[0, 2, 3].item() == -1.0 and x.grad.abs().sum().item() == 1.0


def test_metrics_equal_the_reference_exactly(dev, golden, L):
    from weaklysuperviseddl_amd import ops
    g = golden("lovasz_binary")
    for m in cases(g, "iou"):
        r = L.iou(T(g[m["preds"]]).to(dev), T(g[m["labels"]]).to(dev), m["C"], m["EMPTY"], m["ignore"], m["per_image"])
        assert isinstance(r, np.ndarray) and np.array_equal(r, g[m["case"] + "_result"]), (m, r)
    for m in cases(g, "iou_binary"):
        r = L.iou_binary(T(g[m["preds"]]).to(dev), T(g[m["labels"]]).to(dev), m["EMPTY"], m["ignore"], m["per_image"])
        assert isinstance(r, float) and r == float(g[m["case"] + "_result"]), (m, r)
    # beyond 8 classes the counts go through a histogram in LDS, beyond 512 some of them straight to memory
    gen = torch.Generator().manual_seed(11)
    for C, shape in ((21, (3, 40, 50)), (600, (2, 64, 64))):
        preds, labels = torch.randint(0, C, shape, generator=gen), torch.randint(0, C + 1, shape, generator=gen)
        labels[labels == C] = 255
        for per_image in (False, True):
            got = ops.iou_counts(preds.to(dev), labels.to(dev), C, 255, per_image).cpu().numpy()
            assert np.array_equal(got, O.iou_counts(preds, labels, C, 255, per_image)), (C, per_image)


def test_binary_xloss_and_xloss(dev, golden, L):
    g = golden("lovasz_binary")
    for m in cases(g, "binary_xloss") + cases(g, "xloss"):
        n = m["case"]
        x = T(g[n + "_logits"]).to(dev).requires_grad_()
        lab = T(g[n + "_labels"])
        loss = (L.binary_xloss if m["fn"] == "binary_xloss" else L.xloss)(x, lab.to(dev), m["ignore"])
        loss.backward()
        ref_loss, ref = float(g[n + "_loss"]), T(g[n + "_grad"])
        e_loss = abs(loss.item() - ref_loss) / abs(ref_loss)
        e_grad = ((x.grad.cpu() - ref).abs().max() / ref.abs().max()).item()
        print(f"{n}: loss rel err {e_loss:.3e}, grad rel err {e_grad:.3e}")
        assert e_loss <= 1e-5 and e_grad <= 1e-4, (n, e_loss, e_grad)              # test_cross_entropy's bounds
        void = lab == 255
        if void.any():
            assert (x.grad.cpu()[void if x.dim() == 3 else void.unsqueeze(1).expand(x.shape)] == 0).all()
    # StableBCELoss: float targets, every element counts
    x0, lab = T(g["bce0_logits"]), T(g["bce0_labels"])
    x = x0.to(dev).requires_grad_()
    loss = L.StableBCELoss()(x, lab.float().to(dev))
    loss.backward()
    assert abs(loss.item() - float(g["bce0_loss"])) <= 1e-5 * float(g["bce0_loss"])
    assert ((x.grad.cpu() - T(g["bce0_grad"])).abs().max() / T(g["bce0_grad"]).abs().max()).item() <= 1e-4
    # every pixel void: NaN, as the reference's mean of nothing; the gradient stays zero
    x = torch.randn(2, 5, 5, device=dev, requires_grad=True)
    loss = L.binary_xloss(x, torch.full((2, 5, 5), 255, device=dev), 255)
    loss.backward()
    assert torch.isnan(loss).item() and (x.grad == 0).all()


@pytest.mark.parametrize("shape", [(4, 512, 512), (32, 256, 256)])
@pytest.mark.parametrize("per_image", [True, False])
def test_hinge_full_size_vs_fp32_oracle(dev, shape, per_image):
    """Loss to 1e-5; gradient to 2e-4 of its maximum where the error is distinct within its segment (inside a tie the
    reference's order is whatever torch.sort gave, ours the pixel index - the loss does not depend on it); two runs bit-identical."""
    from weaklysuperviseddl_amd import ops
    gen = torch.Generator().manual_seed(5)
    logits = 2.0 * torch.randn(shape, generator=gen)
    labels = (torch.rand(shape, generator=gen) > 0.6).long()
    lc = logits.clone().requires_grad_()
    lo = O.lovasz_hinge(lc, labels, per_image=per_image)
    lo.backward()
    ld = logits.to(dev).requires_grad_()
    lh = ops.lovasz_hinge(ld, labels.to(dev), per_image=per_image)
    lh.backward()
    err = 1.0 - logits * (2.0 * labels.float() - 1.0)
    distinct = torch.zeros(shape, dtype=torch.bool)
    for seg_e, seg_d in zip(err, distinct) if per_image else [(err, distinct)]:
        _u, inv, cnt = torch.unique(seg_e.reshape(-1), return_inverse=True, return_counts=True)
        seg_d.copy_((cnt[inv] == 1).reshape(seg_e.shape))
    a, b = ld.grad.cpu()[distinct], lc.grad[distinct]
    e_loss = abs(lh.item() - lo.item()) / abs(lo.item())
    e_grad = (a - b).abs().max().item() / b.abs().max().item()
    print(f"hinge {shape} per_image={per_image}: loss {lh.item():.9g} oracle {lo.item():.9g} rel {e_loss:.3e}; "
          f"distinct share {distinct.float().mean().item():.4f}; grad max|d| / max|ref| {e_grad:.3e}")
    assert e_loss <= 1e-5
    assert distinct.float().mean() > 0.5
    assert e_grad <= 2e-4
    ld2 = logits.to(dev).requires_grad_()
    lh2 = ops.lovasz_hinge(ld2, labels.to(dev), per_image=per_image)
    lh2.backward()
    assert lh2.item() == lh.item() and torch.equal(ld2.grad, ld.grad)


def test_hinge_on_two_planes_equals_hinge_on_their_difference(dev):
    from weaklysuperviseddl_amd import ops
    gen = torch.Generator().manual_seed(6)
    z = (2.0 * torch.randn(5, 2, 48, 40, generator=gen)).to(dev)
    labels = torch.randint(0, 2, (5, 48, 40), generator=gen)
    labels[torch.rand(5, 48, 40, generator=gen) < 0.1] = 255
    labels = labels.to(dev)
    for per_image in (True, False):
        z2 = z.clone().requires_grad_()
        d = (z[:, 1] - z[:, 0]).requires_grad_()
        l2, l1 = ops.lovasz_hinge(z2, labels, per_image, 255), ops.lovasz_hinge(d, labels, per_image, 255)
        l2.backward(), l1.backward()
        assert l2.item() == l1.item() and d.grad.abs().max().item() > 0
        assert torch.equal(z2.grad[:, 1], d.grad) and torch.equal(z2.grad[:, 0], -d.grad)


def test_limits_are_refused(dev):
    from weaklysuperviseddl_amd import ops, WsdlError
    x = torch.zeros(1, 4096, 4096, device=dev)                               # a segment of 2^24 pixels
    lab = torch.zeros(1, 4096, 4096, dtype=torch.long, device=dev)
    with pytest.raises(WsdlError, match="2\\^24"):
        ops.lovasz_hinge(x, lab, per_image=True)
    with pytest.raises(WsdlError, match="2\\^24"):
        ops.lovasz_softmax(x, lab, [1], per_image=False)
    with pytest.raises(WsdlError):
        ops.lovasz_softmax(torch.rand(1, 3, 4, 4, device=dev), lab[:, :4, :4].contiguous(), [3])     # not a channel
    with pytest.raises(WsdlError):
        ops.lovasz_hinge(torch.zeros(1, 3, 4, 4, device=dev), lab[:, :4, :4].contiguous())          # three planes
    with pytest.raises(WsdlError):
        ops.lovasz_hinge(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))               # no CPU fallback


def test_train_step_with_lovasz_hinge(dev):
    """loss_fn='lovasz_hinge': the step runs, the loss is finite and falls (the pattern of test_train_step_with_lovasz_softmax)."""
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    import bench
    torch.manual_seed(0)
    model = build_segmentation_model().to(dev).train()
    opt = make_optimizer(model, lr=1e-4)
    img, masks = bench.synthetic_batch(4, 64, 64, dev, 3)
    losses = [float(train_step(model, opt, img, masks, loss_fn="lovasz_hinge")) for _ in range(6)]
    print("lovasz_hinge train losses:", losses)
    assert all(np.isfinite(losses)) and min(losses[2:]) < losses[0], losses
    with pytest.raises(ValueError, match="lovasz_hinge"):
        train_step(model, opt, img, masks, loss_fn="dice")


def test_lovasz_hinge_step_poisons_the_recording(dev):
    """A planned step that contains the hinge cannot be recorded (rocPRIM launches kernels of its own): it is disabled with that
    reason and its results stay the eager path's, bit for bit."""
    from weaklysuperviseddl_amd import plan
    from weaklysuperviseddl_amd.TraditionalModel import build_segmentation_model, train_step
    from weaklysuperviseddl_amd.TraditionalModel.SegmentationModel import make_optimizer
    g = torch.Generator().manual_seed(9)
    img = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    masks = ((torch.rand(2, 64, 64, generator=g) > 0.5).long() * 255).to(dev)

    def run(planned):
        old = plan.PLAN_STEP[0]
        plan.PLAN_STEP[0] = planned
        try:
            torch.manual_seed(0)
            model = build_segmentation_model().to(dev).train()
            opt = make_optimizer(model, lr=1e-4)
            torch.manual_seed(1234)
            losses = [float(train_step(model, opt, img, masks, loss_fn="lovasz_hinge")) for _ in range(4)]
            torch.cuda.synchronize()
            st = next(iter(opt.__dict__.get("_wsdl_planned", {}).values()), None)
            return [opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()] + [b.clone() for b in model.buffers()], losses, st
        finally:
            plan.PLAN_STEP[0] = old

    s0, l0, _ = run(False)
    s1, l1, st = run(True)
    assert st is not None and st.disabled is not None and "recording failed" in st.disabled and "rocPRIM" in st.disabled
    assert "wsdl_lovasz_hinge_fwd_bwd" in st.disabled
    assert l0 == l1
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
