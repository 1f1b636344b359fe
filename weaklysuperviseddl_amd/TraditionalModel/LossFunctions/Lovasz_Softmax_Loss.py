"""The reference's Lovasz loss file on the HIP path (reference TraditionalModel/LossFunctions/Lovasz-Softmax_Loss.py - the
file name there carries a hyphen and cannot be imported as a module; SegmentationModel.py:103-105 calls it as
``lovasz_softmax(F.softmax(outputs, dim=1), masks, classes='present', per_image=False, ignore=None)``).

All fourteen names of that file with their positional signatures and defaults:

- losses: ``lovasz_hinge`` / ``lovasz_hinge_flat`` (binary hinge), ``lovasz_softmax`` / ``lovasz_softmax_flat`` (``classes``
  'present', 'all' or a list of classes), ``binary_xloss`` / ``StableBCELoss``, ``xloss``.  Sorting, the Jaccard gradient
  and the dot products run on the device (csrc/lovasz_seg.hip: the images and list entries are segments of ONE sort,
  'present' / 'all' sort class after class); ties between equal errors are ranked by pixel
  index, the loss does not depend on that order.  The flat variants are the same kernels at B = 1, H = 1, W = P.
- metrics: ``iou_binary`` / ``iou`` - the counts come from the device in one copy, the divisions, the mean and the x 100
  are done on the host with Python floats as in the reference, so the results can be exactly equal.
- tensor plumbing: ``lovasz_grad``, ``flatten_binary_scores``, ``flatten_probas``, ``isnan``, ``mean``.

Where the reference leaves the result undefined: ``lovasz_softmax(per_image=True)`` with an image whose pixels are all void
returns an empty tensor there; here that image is a zero term that counts in the mean, like the hinge's.  A segment with
exactly one valid pixel raises IndexError there; here it is computed.  ``binary_xloss`` with every pixel void is NaN, as in
the reference (the mean of nothing)."""
import torch

from ... import ops


def lovasz_grad(gt_sorted):
    """Jaccard differences along a descending sort: J_k = 1 - (G - cumsum(gt)_k) / (G + cumsum(1 - gt)_k) with G = sum(gt);
    entry k is J_k - J_{k-1}, entry 0 is J_0.  Plain tensor code on the tensor's own device."""
    total = gt_sorted.sum()
    jac = 1.0 - (total - gt_sorted.float().cumsum(0)) / (total + (1 - gt_sorted).float().cumsum(0))
    if len(gt_sorted) > 1:
        jac[1:] = jac[1:] - jac[:-1].clone()
    return jac


def _host_ratios(counts, EMPTY):
    return [float(i) / float(u) if u else EMPTY for i, u in counts]


def iou_binary(preds, labels, EMPTY=1., ignore=None, per_image=True):
    """100 x IoU of the foreground class (1), the mean over the images with ``per_image``; a float."""
    counts = ops.iou_counts(preds.long(), labels.long(), 2, ignore, per_image).cpu()
    return 100 * mean(_host_ratios(counts[:, 1].tolist(), EMPTY))


def iou(preds, labels, C, EMPTY=1., ignore=None, per_image=False):
    """100 x IoU per class as a numpy array, the ``ignore`` class left out."""
    return ops.iou_from_counts(ops.iou_counts(preds.long(), labels.long(), C, ignore, per_image).cpu().numpy(), EMPTY, ignore)


def lovasz_hinge(logits, labels, per_image=True, ignore=None):
    """logits (B,H,W) (or (B,2,H,W): plane 1 - plane 0), labels (B,H,W) in {0, 1, ignore}."""
    return ops.lovasz_hinge(logits, labels.long(), per_image=per_image, ignore=ignore)


def lovasz_hinge_flat(logits, labels):
    """logits (P,), labels (P,) in {0, 1}."""
    if len(labels) == 0:
        return logits.sum() * 0.
    return ops.lovasz_hinge(logits.reshape(1, 1, -1), labels.long().reshape(1, 1, -1), per_image=False, ignore=None)


def flatten_binary_scores(scores, labels, ignore=None):
    """(P,) scores and labels of the batch without the pixels labelled ``ignore``."""
    scores, labels = scores.reshape(-1), labels.reshape(-1)
    if ignore is None:
        return scores, labels
    keep = labels != ignore
    return scores[keep], labels[keep]


class StableBCELoss(torch.nn.Module):
    """mean of max(x,0) - x t + log(1 + exp(-|x|)) over all elements; ``target`` float."""

    def forward(self, input, target):
        return ops.binary_xloss(input, target.float())


def binary_xloss(logits, labels, ignore=None):
    """logits (B,H,W), labels (B,H,W) in {0, 1, ignore}: the stable binary cross entropy over the pixels that are not void."""
    return ops.binary_xloss(logits, labels.long(), ignore)


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None):
    return ops.lovasz_softmax(probas, labels.long(), classes=classes, per_image=per_image, ignore=ignore)


def lovasz_softmax_flat(probas, labels, classes="present"):
    """probas (P,C), labels (P,)."""
    if probas.numel() == 0:
        return probas * 0.
    P, C = probas.shape
    return ops.lovasz_softmax(probas.t().reshape(1, C, 1, P), labels.long().reshape(1, 1, P), classes=classes, per_image=False,
                              ignore=None)


def flatten_probas(probas, labels, ignore=None):
    """(P,C) probabilities and (P,) labels of the batch without the pixels labelled ``ignore``; (B,H,W) is one sigmoid map."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)
    probas = probas.permute(0, 2, 3, 1).reshape(-1, probas.shape[1])
    labels = labels.reshape(-1)
    if ignore is None:
        return probas, labels
    keep = labels != ignore
    return probas[keep], labels[keep]


def xloss(logits, labels, ignore=None):
    """Cross entropy; like the reference it does not look at ``ignore`` and leaves label 255 out."""
    return ops.cross_entropy(logits, labels.long(), 255)


def isnan(x):
    return x != x


def mean(l, ignore_nan=False, empty=0):
    """Mean of an iterable (a generator too), optionally without its NaNs; ``empty`` for none ('raise': ValueError)."""
    vals = [v for v in l if not (ignore_nan and isnan(v))]
    if not vals:
        if empty == "raise":
            raise ValueError("Empty mean")
        return empty
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    return acc if len(vals) == 1 else acc / len(vals)
