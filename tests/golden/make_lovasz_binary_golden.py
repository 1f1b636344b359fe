#!/usr/bin/env python3
"""Generate tests/golden/lovasz_binary.npz from the reference's own function bodies - the recipe of make_golden.py: the
reference file (LossFunctions/Lovasz-Softmax_Loss.py, torch + numpy only) cannot be imported under its hyphenated name, so
its top-level FunctionDef / ClassDef nodes are selected by name with ``ast`` and executed in a namespace that provides
torch / F / np / Variable.  Runs ONLY in the build container (needs /root/reference).  Nothing of the reference's text is
written to the fixture: it holds seeded inputs and the outputs the reference bodies produced for them.

    python tests/golden/make_lovasz_binary_golden.py

Cases (meta is a JSON list; arrays are named ``<case>_<what>``):
  hinge     lovasz_hinge, per image and whole batch x {no ignore, ignore 255, one image all void}
  softmax   lovasz_softmax with the class lists [1] and [0, 2], per image with an ignored label, one sigmoid map with [1]
  iou       iou / iou_binary with and without ignore, ignore = 2 inside the class range, a class nobody has (EMPTY)
  bce       binary_xloss with and without ignore;  xloss
Inputs are tie-free (checked): the gradient then does not depend on how a sort orders equal errors.
"""
import ast
import json
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Variable

try:
    from itertools import ifilterfalse
except ImportError:
    from itertools import filterfalse as ifilterfalse

REF = "/root/reference/TraditionalModel/LossFunctions/Lovasz-Softmax_Loss.py"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {"lovasz_grad", "iou_binary", "iou", "lovasz_hinge", "lovasz_hinge_flat", "flatten_binary_scores", "StableBCELoss",
         "binary_xloss", "lovasz_softmax", "lovasz_softmax_flat", "flatten_probas", "xloss", "isnan", "mean"}


def lift():
    tree = ast.parse(open(REF).read())
    picked = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in NAMES]
    assert {n.name for n in picked} == NAMES
    ns = {"torch": torch, "F": F, "np": np, "Variable": Variable, "ifilterfalse": ifilterfalse}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # ``classes is 'present'``: SyntaxWarning
        exec(compile(ast.Module(body=picked, type_ignores=[]), REF, "exec"), ns)
    return ns


def distinct(t):
    return torch.unique(t.reshape(-1)).numel() == t.numel()


def main():
    ns = lift()
    out, meta = {}, []

    # ---- hinge
    B, H, W = 3, 12, 20
    for i, (per_image, kind) in enumerate([(p, k) for p in (True, False) for k in ("plain", "ignore", "void_image")]):
        g = torch.Generator().manual_seed(700 + i)
        logits = (2.0 * torch.randn(B, H, W, generator=g)).requires_grad_()
        labels = torch.randint(0, 2, (B, H, W), generator=g)
        ignore = None
        if kind != "plain":
            ignore = 255
            labels[torch.rand(B, H, W, generator=g) < 0.15] = 255
        if kind == "void_image":
            labels[1] = 255
        assert distinct(1.0 - logits.detach() * (2.0 * labels.float() - 1.0))
        loss = ns["lovasz_hinge"](logits, labels, per_image=per_image, ignore=ignore)
        loss.backward()
        name = f"hinge{i}"
        out[f"{name}_logits"], out[f"{name}_labels"] = logits.detach().numpy(), labels.numpy()
        out[f"{name}_loss"], out[f"{name}_grad"] = np.float64(loss.item()), logits.grad.numpy()
        meta.append(dict(case=name, fn="lovasz_hinge", per_image=per_image, ignore=ignore, kind=kind))

    # ---- softmax with a class list
    cases = [("softmax0", 3, [1], False, None), ("softmax1", 3, [0, 2], False, None), ("softmax2", 3, [0, 2], True, 255),
             ("softmax3", 3, [1], True, None), ("softmax4", 0, [1], False, None), ("softmax5", 0, [1], True, 255)]
    for i, (name, C, classes, per_image, ignore) in enumerate(cases):
        g = torch.Generator().manual_seed(720 + i)
        B, H, W = 3, 10, 12
        if C:
            probas = F.softmax(1.5 * torch.randn(B, C, H, W, generator=g), dim=1).detach().requires_grad_()
            labels = torch.randint(0, C, (B, H, W), generator=g)
        else:                                                  # one sigmoid map (B,H,W); foreground = labels == 1
            probas = torch.sigmoid(1.5 * torch.randn(B, H, W, generator=g)).detach().requires_grad_()
            labels = torch.randint(0, 2, (B, H, W), generator=g)
        if ignore is not None:
            labels[torch.rand(B, H, W, generator=g) < 0.15] = ignore
        pd = probas.detach() if C else probas.detach().unsqueeze(1)
        for c in classes:
            assert distinct(((labels == c).float() - pd[:, c if C else 0]).abs())
        loss = ns["lovasz_softmax"](probas, labels, classes=classes, per_image=per_image, ignore=ignore)
        loss.backward()
        out[f"{name}_probas"], out[f"{name}_labels"] = probas.detach().numpy(), labels.numpy()
        out[f"{name}_loss"], out[f"{name}_grad"] = np.float64(loss.item()), probas.grad.numpy()
        meta.append(dict(case=name, fn="lovasz_softmax", classes=classes, per_image=per_image, ignore=ignore, sigmoid=not C))

    # ---- metrics
    g = torch.Generator().manual_seed(740)
    B, H, W, C = 3, 9, 11, 4
    preds = torch.randint(0, C, (B, H, W), generator=g)
    labels = torch.randint(0, C, (B, H, W), generator=g)
    lab255 = labels.clone()
    lab255[torch.rand(B, H, W, generator=g) < 0.2] = 255
    no3 = labels.clone()
    no3[no3 == 3] = 0                                           # class 3 in no label ...
    p_no3 = preds.clone()
    p_no3[p_no3 == 3] = 1                                       # ... and in no prediction: union 0 -> EMPTY
    bp, bl = (preds > 1).long(), (labels > 1).long()
    bl255 = bl.clone()
    bl255[lab255 == 255] = 255
    out["iou_preds"], out["iou_labels"], out["iou_labels255"] = preds.numpy(), labels.numpy(), lab255.numpy()
    out["iou_preds_no3"], out["iou_labels_no3"] = p_no3.numpy(), no3.numpy()
    out["ioub_preds"], out["ioub_labels"], out["ioub_labels255"] = bp.numpy(), bl.numpy(), bl255.numpy()
    out["ioub_zeros"] = np.zeros((B, H, W), np.int64)
    k = 0
    for (pk, lk, EMPTY, ignore) in [("iou_preds", "iou_labels", 1.0, None), ("iou_preds", "iou_labels255", 1.0, 255),
                                    ("iou_preds", "iou_labels", 1.0, 2), ("iou_preds_no3", "iou_labels_no3", 0.5, None)]:
        for per_image in (False, True):
            r = ns["iou"](torch.from_numpy(out[pk]), torch.from_numpy(out[lk]), C, EMPTY, ignore, per_image)
            out[f"iou{k}_result"] = np.asarray(r, np.float64)
            meta.append(dict(case=f"iou{k}", fn="iou", preds=pk, labels=lk, C=C, EMPTY=EMPTY, ignore=ignore, per_image=per_image))
            k += 1
    k = 0
    for (pk, lk, EMPTY, ignore) in [("ioub_preds", "ioub_labels", 1.0, None), ("ioub_preds", "ioub_labels255", 1.0, 255),
                                    ("ioub_zeros", "ioub_zeros", 0.25, None)]:
        for per_image in (True, False):
            r = ns["iou_binary"](torch.from_numpy(out[pk]), torch.from_numpy(out[lk]), EMPTY, ignore, per_image)
            out[f"ioub{k}_result"] = np.float64(r)
            meta.append(dict(case=f"ioub{k}", fn="iou_binary", preds=pk, labels=lk, EMPTY=EMPTY, ignore=ignore, per_image=per_image))
            k += 1

    # ---- binary cross entropy, cross entropy
    for i, ignore in enumerate((None, 255)):
        g = torch.Generator().manual_seed(760 + i)
        logits = (3.0 * torch.randn(3, 12, 20, generator=g)).requires_grad_()
        labels = torch.randint(0, 2, (3, 12, 20), generator=g)
        if ignore is not None:
            labels[torch.rand(3, 12, 20, generator=g) < 0.2] = ignore
        loss = ns["binary_xloss"](logits, labels, ignore)
        loss.backward()
        out[f"bce{i}_logits"], out[f"bce{i}_labels"] = logits.detach().numpy(), labels.numpy()
        out[f"bce{i}_loss"], out[f"bce{i}_grad"] = np.float64(loss.item()), logits.grad.numpy()
        meta.append(dict(case=f"bce{i}", fn="binary_xloss", ignore=ignore))
    g = torch.Generator().manual_seed(770)
    logits = (2.0 * torch.randn(2, 3, 8, 10, generator=g)).requires_grad_()
    labels = torch.randint(0, 3, (2, 8, 10), generator=g)
    labels[torch.rand(2, 8, 10, generator=g) < 0.2] = 255
    loss = ns["xloss"](logits, labels, ignore=7)               # the argument is not looked at: 255 is what is left out
    loss.backward()
    out["xloss0_logits"], out["xloss0_labels"] = logits.detach().numpy(), labels.numpy()
    out["xloss0_loss"], out["xloss0_grad"] = np.float64(loss.item()), logits.grad.numpy()
    meta.append(dict(case="xloss0", fn="xloss", ignore=7))

    out["meta"] = np.array(json.dumps(meta))
    path = f"{HERE}/lovasz_binary.npz"
    np.savez_compressed(path, **out)
    print("lovasz_binary.npz", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
