"""The binary half of the reference's Lovasz file without a GPU: the fp32 oracle (tests/lovasz_binary_oracle.py) against the
vectors the reference's own function bodies produced (tests/golden/lovasz_binary.npz, made by
tests/golden/make_lovasz_binary_golden.py), the host arithmetic of the IoU metrics, and the public surfaces - the drop-in
module's fourteen names and the C ABI's new entries."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_binary_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def cases(g, fn):
    return [m for m in json.loads(str(g["meta"])) if m["fn"] == fn]


def test_fixture_holds_the_cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "lovasz_binary.npz"), allow_pickle=False)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lovasz_binary.npz")) < 200 * 1024
    h = {(m["per_image"], m["kind"]) for m in cases(g, "lovasz_hinge")}
    assert h == {(p, k) for p in (True, False) for k in ("plain", "ignore", "void_image")}
    s = cases(g, "lovasz_softmax")
    assert any(m["classes"] == [1] and not m["sigmoid"] for m in s) and any(m["classes"] == [0, 2] for m in s)
    assert any(m["per_image"] and m["ignore"] is not None for m in s) and any(m["sigmoid"] and m["classes"] == [1] for m in s)
    i = cases(g, "iou")
    assert any(m["ignore"] is None for m in i) and any(m["ignore"] == 255 for m in i) and any(m["ignore"] == 2 for m in i)
    assert any(m["EMPTY"] != 1.0 for m in i) and any(m["EMPTY"] != 1.0 for m in cases(g, "iou_binary"))
    assert {m["ignore"] for m in cases(g, "binary_xloss")} == {None, 255} and cases(g, "xloss")
    # tie-free hinge inputs: the gradient does not depend on how a sort orders equal errors
    for m in cases(g, "lovasz_hinge"):
        lg, lb = g[m["case"] + "_logits"], g[m["case"] + "_labels"]
        e = 1.0 - lg * (2.0 * lb.astype(np.float32) - 1.0)
        assert np.unique(e).size == e.size


def test_oracle_losses_against_the_reference_vectors(golden):
    """Loss and gradient at rel = 1e-5, the yardstick of test_lovasz_softmax_loss_and_grad."""
    g = golden("lovasz_binary")
    for m in cases(g, "lovasz_hinge") + cases(g, "lovasz_softmax") + cases(g, "binary_xloss") + cases(g, "xloss"):
        n = m["case"]
        x = T(g[n + ("_probas" if m["fn"] == "lovasz_softmax" else "_logits")]).requires_grad_()
        lab = T(g[n + "_labels"])
        if m["fn"] == "lovasz_hinge":
            loss = O.lovasz_hinge(x, lab, per_image=m["per_image"], ignore=m["ignore"])
        elif m["fn"] == "lovasz_softmax":
            loss = O.lovasz_softmax(x, lab, m["classes"], per_image=m["per_image"], ignore=m["ignore"])
        elif m["fn"] == "binary_xloss":
            loss = O.binary_xloss(x, lab, m["ignore"])
        else:
            loss = O.xloss(x, lab, m["ignore"])
        loss.backward()
        assert loss.item() == pytest.approx(float(g[n + "_loss"]), rel=1e-5), n
        ref = g[n + "_grad"]
        assert np.allclose(x.grad.numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), n
        if m.get("ignore") is not None and m["fn"] != "xloss":
            void = (lab == m["ignore"])
            if m["fn"] == "lovasz_softmax" and x.dim() == 4:
                void = void.unsqueeze(1).expand_as(x)
            assert void.any() and (x.grad[void] == 0).all(), n


def test_all_void_and_sigmoid_list_semantics():
    lg = torch.randn(2, 4, 5, requires_grad=True)
    void = torch.full((2, 4, 5), 255)
    for per_image in (True, False):
        loss = O.lovasz_hinge(lg, void, per_image=per_image, ignore=255)
        assert loss.item() == 0.0
    with pytest.raises(ValueError):
        O.lovasz_softmax(torch.rand(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.long), [0, 1])
    assert torch.isnan(O.binary_xloss(lg, void, 255))


def test_oracle_metrics_equal_the_reference_exactly(golden):
    g = golden("lovasz_binary")
    for m in cases(g, "iou"):
        r = O.iou(T(g[m["preds"]]), T(g[m["labels"]]), m["C"], m["EMPTY"], m["ignore"], m["per_image"])
        assert r.shape == g[m["case"] + "_result"].shape and np.array_equal(r, g[m["case"] + "_result"]), m
        assert len(r) == m["C"] - (1 if m["ignore"] is not None and m["ignore"] < m["C"] else 0)
    for m in cases(g, "iou_binary"):
        r = O.iou_binary(T(g[m["preds"]]), T(g[m["labels"]]), m["EMPTY"], m["ignore"], m["per_image"])
        assert isinstance(r, float) and r == float(g[m["case"] + "_result"]), m


def test_iou_from_counts_against_the_reference_from_host_counts(golden):
    """ops.iou_from_counts is pure host arithmetic: fed with counts made on the host it gives the reference's numbers exactly."""
    from weaklysuperviseddl_amd import ops
    g = golden("lovasz_binary")
    for m in cases(g, "iou"):
        counts = O.iou_counts(T(g[m["preds"]]), T(g[m["labels"]]), m["C"], m["ignore"], m["per_image"])
        r = ops.iou_from_counts(counts, m["EMPTY"], m["ignore"])
        assert r.dtype == np.float64 and np.array_equal(r, g[m["case"] + "_result"]), m
        r = ops.iou_from_counts(torch.from_numpy(counts), m["EMPTY"], m["ignore"])          # a host tensor too
        assert np.array_equal(r, g[m["case"] + "_result"]), m


def test_module_exports_the_fourteen_names_with_the_reference_signatures():
    """The reference's ``def`` lines (LossFunctions/Lovasz-Softmax_Loss.py, cited), restated here: the reference does not
    travel with the tests."""
    import inspect
    from weaklysuperviseddl_amd.TraditionalModel.LossFunctions import Lovasz_Softmax_Loss as L
    P = inspect.Parameter
    want = {
        "lovasz_grad": [("gt_sorted", P.empty)],                                                                  # :11
        "iou_binary": [("preds", P.empty), ("labels", P.empty), ("EMPTY", 1.), ("ignore", None), ("per_image", True)],   # :26
        "iou": [("preds", P.empty), ("labels", P.empty), ("C", P.empty), ("EMPTY", 1.), ("ignore", None), ("per_image", False)],  # :46
        "lovasz_hinge": [("logits", P.empty), ("labels", P.empty), ("per_image", True), ("ignore", None)],        # :71
        "lovasz_hinge_flat": [("logits", P.empty), ("labels", P.empty)],                                          # :87
        "flatten_binary_scores": [("scores", P.empty), ("labels", P.empty), ("ignore", None)],                    # :107
        "binary_xloss": [("logits", P.empty), ("labels", P.empty), ("ignore", None)],                             # :131
        "lovasz_softmax": [("probas", P.empty), ("labels", P.empty), ("classes", "present"), ("per_image", False),
                           ("ignore", None)],                                                                     # :146
        "lovasz_softmax_flat": [("probas", P.empty), ("labels", P.empty), ("classes", "present")],                # :164
        "flatten_probas": [("probas", P.empty), ("labels", P.empty), ("ignore", None)],                           # :195
        "xloss": [("logits", P.empty), ("labels", P.empty), ("ignore", None)],                                    # :213
        "isnan": [("x", P.empty)],                                                                                # :221
        "mean": [("l", P.empty), ("ignore_nan", False), ("empty", 0)],                                            # :225
    }
    for name, params in want.items():
        got = list(inspect.signature(getattr(L, name)).parameters.values())
        assert [(p.name, p.default) for p in got] == params, (name, [(p.name, p.default) for p in got])
        assert all(p.kind == P.POSITIONAL_OR_KEYWORD for p in got), name
    # :122-128  class StableBCELoss(torch.nn.modules.Module): __init__(self), forward(self, input, target)
    assert issubclass(L.StableBCELoss, torch.nn.Module)
    L.StableBCELoss()                                        # no constructor arguments
    assert list(inspect.signature(L.StableBCELoss.forward).parameters) == ["self", "input", "target"]
    # the plumbing runs on host tensors
    assert L.mean([1.0, 2.0, 6.0]) == 3.0 and L.mean(iter([])) == 0 and L.mean([float("nan"), 2.0], ignore_nan=True) == 2.0
    with pytest.raises(ValueError):
        L.mean([], empty="raise")
    assert L.isnan(float("nan")) and not L.isnan(1.0)
    gt = torch.tensor([1, 0, 1, 1, 0])
    assert torch.equal(L.lovasz_grad(gt), O.jaccard_steps(gt))
    s, l = L.flatten_binary_scores(torch.arange(6.).view(1, 2, 3), torch.tensor([[[0, 255, 1], [1, 0, 255]]]), 255)
    assert s.tolist() == [0., 2., 3., 4.] and l.tolist() == [0, 1, 1, 0]
    p, l = L.flatten_probas(torch.arange(12.).view(1, 2, 2, 3), torch.tensor([[[0, 9, 1], [1, 0, 9]]]), 9)
    assert p.tolist() == [[0., 6.], [2., 8.], [3., 9.], [4., 10.]] and l.tolist() == [0, 1, 1, 0]


def test_new_symbols_are_in_the_header_and_bound():
    from weaklysuperviseddl_amd import _lib
    src = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    for name in ("wsdl_lovasz_hinge_workspace", "wsdl_lovasz_hinge_fwd_bwd", "wsdl_lovasz_softmax_classes_workspace",
                 "wsdl_lovasz_softmax_classes_fwd_bwd", "wsdl_iou_counts", "wsdl_binary_xloss_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    for cite in ("Lovasz-Softmax_Loss.py:26-65", "Lovasz-Softmax_Loss.py:71-119", "Lovasz-Softmax_Loss.py:122-140",
                 "Lovasz-Softmax_Loss.py:146-211"):
        assert cite in src, cite
    # the note at wsdl_plan_begin names the entries that poison a recording
    note = src[src.index("launch plans"):src.index("int wsdl_plan_begin(void);")]
    assert "wsdl_lovasz_hinge_fwd_bwd" in note and "wsdl_lovasz_softmax_classes_fwd_bwd" in note


def test_null_pointers_are_refused_on_the_host():
    """Checked before anything touches a device (the size limits need rocPRIM's size query, which needs one: GPU tests)."""
    from weaklysuperviseddl_amd import _lib
    lib = _lib.lib()
    assert lib.wsdl_lovasz_hinge_fwd_bwd(None, None, None, None, 1, 1, 8, 8, 1, -1, None, 0, None) != 0
    assert b"null pointer" in lib.wsdl_last_error()
    assert lib.wsdl_lovasz_softmax_classes_fwd_bwd(None, None, None, None, 1, 2, 8, 8, None, 1, 1, -1, None, 0, None) != 0
    assert b"null pointer" in lib.wsdl_last_error()
    assert lib.wsdl_iou_counts(None, None, None, 1, 64, 2, 1, -1, None) != 0 and b"null pointer" in lib.wsdl_last_error()
    assert lib.wsdl_binary_xloss_fwd_bwd(None, None, None, None, None, None, 64, -1, None, 0, None) != 0
    assert b"null pointer" in lib.wsdl_last_error()
    assert lib.wsdl_lovasz_hinge_workspace(0, 8, 8, 1) == 0 and lib.wsdl_lovasz_softmax_classes_workspace(8, 3, 8, 8, 0, 1) == 0


def test_train_entry_points_name_the_third_loss():
    from weaklysuperviseddl_amd.TraditionalModel import train_segmentation_model
    with pytest.raises(ValueError, match="lovasz_hinge"):
        train_segmentation_model("dice", "none")
