"""The tie-stable Lovasz-softmax oracle (tests/lovasz_softmax_oracle.py) without a GPU: pinned to the vectors the reference's
own function bodies produced (tests/golden/lovasz.npz, and the class-list cases of tests/golden/lovasz_binary.npz), bit for bit
to oracle.lovasz_softmax where no two errors are equal, to its loss where they are, and to an invariant of the gradient that
holds for ANY order inside a tie - so the oracle that the GPU tests (tests/test_hip_lovasz_softmax.py) trust is itself held."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_softmax_oracle as S  # noqa: E402

T = torch.from_numpy


def tie_free(p, labels, classes, ignore=None, per_image=False):
    """No two valid pixels of a sorted segment (an image, or the batch) share an error."""
    for pp, ll in zip(p, labels) if per_image else [(p.transpose(0, 1), labels)]:
        pp, ll = pp.reshape(pp.shape[0], -1), ll.reshape(-1)             # (C, pixels of the segment)
        keep = torch.ones_like(ll, dtype=torch.bool) if ignore is None else ll != ignore
        for c in classes:
            e = ((ll == c).float() - pp[c]).abs()[keep]
            if torch.unique(e).numel() != e.numel():
                return False
    return True


def test_oracle_equals_the_reference_vectors(golden):
    """tests/golden/lovasz.npz at the tolerances of test_lovasz_softmax_vs_golden_and_oracle."""
    g = golden("lovasz")
    meta = json.loads(str(g["meta"]))
    assert len(meta) == 6
    for i, m in enumerate(meta):
        loss, grad = S.loss_and_grad(T(g[f"lov{i}_probas"]), T(g[f"lov{i}_labels"]), m["classes"], m["per_image"], m["ignore"])
        ref_loss, ref = float(g[f"lov{i}_loss"]), T(g[f"lov{i}_grad"])
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (i, loss, ref_loss)
        assert (grad - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-9, i


def test_oracle_equals_the_class_list_vectors(golden):
    """The class-list cases test_hip_lovasz_binary.py reads, at its tolerances (check_loss_and_grad there)."""
    g = golden("lovasz_binary")
    cases = [m for m in json.loads(str(g["meta"])) if m["fn"] == "lovasz_softmax"]
    assert any(m["sigmoid"] for m in cases) and any(m["per_image"] and m["ignore"] is not None for m in cases)
    for m in cases:
        n = m["case"]
        p, lab = T(g[n + "_probas"]), T(g[n + "_labels"])
        loss, grad = S.loss_and_grad(p, lab, m["classes"], m["per_image"], m["ignore"])
        ref_loss, ref = float(g[n + "_loss"]), T(g[n + "_grad"])
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (n, loss, ref_loss)
        assert (grad - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-9, n
        if m["ignore"] is not None:
            void = (lab == m["ignore"]) if p.dim() == 3 else (lab == m["ignore"]).unsqueeze(1).expand(p.shape)
            assert void.any() and (grad[void] == 0).all(), n


def test_oracle_is_the_repository_oracle_bit_for_bit_without_ties(golden):
    """Where no two errors are equal a stable sort and any other sort give one order: the same bits, loss and gradient."""
    import oracle
    g = golden("lovasz")
    inputs = []
    for i, m in enumerate(json.loads(str(g["meta"]))):
        inputs.append((T(g[f"lov{i}_probas"]), T(g[f"lov{i}_labels"]), m["classes"], m["per_image"], m["ignore"]))
    gen = torch.Generator().manual_seed(21)
    p = torch.softmax(torch.randn(2, 5, 17, 19, generator=gen), 1)
    lab = torch.randint(0, 4, (2, 17, 19), generator=gen)                  # class 4 absent
    lab[torch.rand(2, 17, 19, generator=gen) < 0.1] = 255
    inputs += [(p, lab, "present", False, 255), (p, lab, "all", False, 255), (p, lab, "present", True, 255),
               (p, lab, [3, 0], False, 255), (p, lab, "all", False, None)]
    checked = 0
    for p, lab, classes, per_image, ignore in inputs:
        listed = range(p.shape[1]) if isinstance(classes, str) else classes
        if not tie_free(p, lab, listed, ignore, per_image):
            continue
        checked += 1
        loss, grad = S.loss_and_grad(p, lab, classes, per_image, ignore)
        pr = p.clone().requires_grad_()
        want = oracle.lovasz_softmax(pr, lab, classes=classes, per_image=per_image, ignore=ignore)
        want.backward()
        assert loss == want.item() and torch.equal(grad, pr.grad), (classes, per_image, ignore)
    assert checked >= 9, checked


def tied_inputs():
    gen = torch.Generator().manual_seed(22)
    out = []
    for shape in ((2, 3, 9, 13), (1, 2, 1, 300)):
        B, C, H, W = shape
        lab = torch.randint(0, C, (B, H, W), generator=gen)
        for name, p in (("eighths", S.quantised_probas(shape, gen)), ("one-hot", S.one_hot_probas(shape, gen))):
            out.append((f"{name} {shape}", p, lab, None))
            void = lab.clone()
            void[torch.rand(B, H, W, generator=gen) < 0.2] = 255
            out.append((f"{name} {shape} void", p, void, 255))
    return out


def test_loss_with_ties_equals_the_repository_oracle():
    """The loss does not depend on the order inside a tie: 1e-6 relative to oracle.lovasz_softmax, whatever its sort did."""
    import oracle
    for name, p, lab, ignore in tied_inputs():
        assert (p == 0).any() and (p == 1).any(), name
        assert not tie_free(p, lab, range(p.shape[1]), ignore), name
        for classes in ("present", "all", [1, 0]):
            for per_image in (False, True):
                got = S.lovasz_softmax(p, lab, classes, per_image, ignore).item()
                want = oracle.lovasz_softmax(p, lab, classes=classes, per_image=per_image, ignore=ignore).item()
                assert abs(got - want) <= 1e-6 * abs(want), (name, classes, per_image, got, want)


def test_gradient_mass_of_every_tie_group():
    """Whatever order a sort gives the members of a tie, their Jaccard steps telescope: over the pixels of class plane c whose
    error is v > 0, sum |d loss / d p| = w (J_after - J_before), J taken after all errors >= v resp. > v (0 for none) and
    w = 1 / (number of classes averaged).  (Error 0 has a zero derivative: |x|' = 0 at 0.)  J is evaluated here in float64
    from the counts; the oracle's fp32 J_k are each within 2 x 2^-24 of it (one rounding in the division, one in 1 - q), each
    of the n differences rounds once more (2^-24) and so does each product with w: bound w (2 n + 4) 2^-24 per group."""
    worst = 0.0
    for name, p, lab, ignore in tied_inputs():
        C = p.shape[1]
        _loss, grad = S.loss_and_grad(p, lab, "all", False, ignore)
        pf, lf = p.transpose(0, 1).reshape(C, -1), lab.reshape(-1)
        gf = grad.transpose(0, 1).reshape(C, -1)
        keep = torch.ones_like(lf, dtype=torch.bool) if ignore is None else lf != ignore
        assert (gf[:, ~keep] == 0).all(), name
        groups = 0
        for c in range(C):
            fg = (lf == c)[keep]
            e = (fg.float() - pf[c][keep]).abs()
            a = gf[c][keep].abs().double()
            G = float(fg.sum())

            def J(sel):
                F, N = float((fg & sel).sum()), float((~fg & sel).sum())
                return 1.0 - (G - F) / (G + N) if G + N > 0 else 0.0
            assert (a[e == 0] == 0).all(), (name, c)
            for v in torch.unique(e[e > 0]).tolist():
                n = int((e == v).sum())
                want = (J(e >= v) - J(e > v)) / C
                bound = (2 * n + 4) * 2.0 ** -24 / C
                err = abs(a[e == v].sum().item() - want)
                worst = max(worst, err / bound)
                assert err <= bound, (name, c, v, n, err, bound)
                groups += n > 1
        assert groups >= 2, (name, groups)
    print(f"tie groups: worst |sum - w dJ| / bound {worst:.3f}")


def test_empty_input_conventions():
    p = torch.rand(2, 3, 4, 5).requires_grad_()
    void = torch.full((2, 4, 5), 255)
    for classes in ("present", "all", [0, 2]):
        for per_image in (False, True):
            p.grad = None
            loss = S.lovasz_softmax(p, void, classes, per_image, 255)
            loss.backward()
            assert loss.item() == 0.0 and (p.grad == 0).all(), (classes, per_image)
    lab = torch.full((2, 4, 5), 7)                           # valid pixels, no class of [0, 3) present
    assert S.lovasz_softmax(p, lab, "present").item() == 0.0 and S.lovasz_softmax(p, lab, "all").item() > 0.0
    half = void.clone()
    half[0] = 1                                              # an all-void image is a zero term that counts in the mean
    one = S.lovasz_softmax(p[:1], half[:1], [1], True, 255).item()
    assert S.lovasz_softmax(p, half, [1], True, 255).item() == pytest.approx(one / 2, rel=1e-6)
    with pytest.raises(ValueError):
        S.lovasz_softmax(torch.rand(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.long), [0, 1])
    m = torch.rand(2, 4, 5)
    lab = torch.randint(0, 2, (2, 4, 5))
    assert S.lovasz_softmax(m, lab, [1]).item() == S.lovasz_softmax(m.unsqueeze(1), lab, [1]).item()
