"""fp32 torch-CPU oracle for the binary half of the reference's Lovasz file (LossFunctions/Lovasz-Softmax_Loss.py: hinge
:71-119, class lists of lovasz_softmax :146-211, iou / iou_binary :26-65, binary_xloss :122-140, xloss :213-217): the same
operations in the same order, restated.  The Jaccard terms stay in float32 on purpose - the reference's own fp32 gradient
lies up to 3.7e-2 of max|grad| away from a float64 restatement at 4 x 512 x 512 (J sits a few ulps under 1), so parity
means its fp32 steps, not more digits.  Pinned to the reference's outputs by tests/test_lovasz_binary.py."""
import numpy as np
import torch
import torch.nn.functional as F


def jaccard_steps(gt_sorted):
    """gt_sorted: 0/1 along a descending sort -> J_k - J_{k-1} (J_{-1} = 0), J_k = 1 - (G - cumsum gt) / (G + cumsum (1 - gt))."""
    G = gt_sorted.sum()
    inter = G - gt_sorted.float().cumsum(0)
    union = G + (1 - gt_sorted).float().cumsum(0)
    J = 1.0 - inter / union
    if J.numel() > 1:
        J = torch.cat([J[:1], J[1:] - J[:-1]])
    return J


def _average(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc if len(terms) == 1 else acc / len(terms)


def hinge_flat(logits, labels):
    """logits (P,), labels (P,) in {0,1} (void pixels already removed)."""
    if labels.numel() == 0:
        return logits.sum() * 0.0
    signs = 2.0 * labels.float() - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
    return torch.dot(F.relu(errors_sorted), jaccard_steps(labels[perm]).detach())


def lovasz_hinge(logits, labels, per_image=True, ignore=None):
    def flat(lg, lb):
        lg, lb = lg.reshape(-1), lb.reshape(-1)
        if ignore is None:
            return lg, lb
        keep = lb != ignore
        return lg[keep], lb[keep]
    if per_image:
        return _average([hinge_flat(*flat(lg, lb)) for lg, lb in zip(logits, labels)])
    return hinge_flat(*flat(logits, labels))


def softmax_flat(probas, labels, classes):
    """probas (P,C), labels (P,), classes a list: every entry is a term whether or not the class occurs."""
    if probas.numel() == 0:
        return probas.sum() * 0.0            # defined here as a zero term (the reference: an empty tensor)
    C = probas.shape[1]
    if C == 1 and len(classes) > 1:
        raise ValueError("Sigmoid output possible only with 1 class")
    terms = []
    for c in classes:
        fg = (labels == c).float()
        errors = (fg - probas[:, 0 if C == 1 else c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        terms.append(torch.dot(errors_sorted, jaccard_steps(fg[perm]).detach()))
    return _average(terms)


def lovasz_softmax(probas, labels, classes, per_image=False, ignore=None):
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)

    def flat(p, l):
        p = p.permute(0, 2, 3, 1).reshape(-1, p.shape[1])
        l = l.reshape(-1)
        if ignore is None:
            return p, l
        keep = l != ignore
        return p[keep], l[keep]
    if per_image:
        return _average([softmax_flat(*flat(p.unsqueeze(0), l.unsqueeze(0)), classes) for p, l in zip(probas, labels)])
    return softmax_flat(*flat(probas, labels), classes)


def iou_counts(preds, labels, C, ignore=None, per_image=False):
    """Host-made (images, C, 2) int64 counts: intersection (label = c and pred = c), union (label = c or (pred = c and not void))."""
    if not per_image:
        preds, labels = preds.reshape(1, -1), labels.reshape(1, -1)
    out = np.zeros((preds.shape[0], C, 2), np.int64)
    for b, (p, l) in enumerate(zip(preds, labels)):
        not_void = torch.ones_like(l, dtype=torch.bool) if ignore is None else l != ignore
        for c in range(C):
            out[b, c, 0] = int(((l == c) & (p == c)).sum())
            out[b, c, 1] = int(((l == c) | ((p == c) & not_void)).sum())
    return out


def iou(preds, labels, C, EMPTY=1.0, ignore=None, per_image=False):
    counts = iou_counts(preds, labels, C, ignore, per_image)
    res = []
    for c in range(C):
        if c == ignore:
            continue
        res.append(_average([float(i) / float(u) if u else EMPTY for i, u in counts[:, c].tolist()]))
    return 100 * np.array(res)


def iou_binary(preds, labels, EMPTY=1.0, ignore=None, per_image=True):
    counts = iou_counts(preds, labels, 2, ignore, per_image)
    return 100 * _average([float(i) / float(u) if u else EMPTY for i, u in counts[:, 1].tolist()])


def binary_xloss(logits, labels, ignore=None):
    x, t = logits.reshape(-1), labels.reshape(-1)
    if ignore is not None:
        keep = t != ignore
        x, t = x[keep], t[keep]
    t = t.float()
    return (x.clamp(min=0) - x * t + (1 + (-x.abs()).exp()).log()).mean()


def xloss(logits, labels, ignore=None):
    return F.cross_entropy(logits, labels, ignore_index=255)
