"""fp32 torch-CPU oracle for the multi-class Lovasz-softmax with a FIXED tie order: oracle/losses.py::lovasz_softmax restated,
the same operations in the same order, with one difference - the sort is ``torch.sort(..., descending=True, stable=True)``,
applied after the void pixels have been removed.  Equal errors then stay in pixel order, which is the order the kernels
document (csrc/lovasz_seg.hip: a stable radix sort over the pixel index), so the WHOLE gradient is
comparable, the pixels inside a tie included.  The loss does not depend on the order inside a tie; the gradient does.

The Jaccard terms stay in float32 on purpose: tests/lovasz_binary_oracle.py explains why a float64 restatement is the wrong
reference (the reference's own fp32 gradient lies up to 3.7e-2 of max|grad| away from it at 4 x 512 x 512).

``classes``: 'present', 'all' or a list; a list with one sigmoid map (C == 1, probas (B,H,W) or (B,1,H,W)) has exactly one
entry c and compares channel 0 with ``labels == c``.  Empty input follows the repository's conventions: a flat input without
a valid pixel is a zero term (that still counts in a per-image mean), 'present' with no class present is 0.
Pinned by tests/test_lovasz_softmax.py."""
import torch


def lovasz_grad(gt_sorted):
    """J_k - J_{k-1} (J_{-1} = 0), J_k = 1 - (G - cumsum(gt)_k) / (G + cumsum(1 - gt)_k): oracle/losses.py::lovasz_grad."""
    gt = gt_sorted.float()
    total = gt.sum()
    inter = total - gt.cumsum(0)
    union = total + (1.0 - gt).cumsum(0)
    jac = 1.0 - inter / union
    out = jac.clone()
    out[1:] = jac[1:] - jac[:-1]
    return out


def lovasz_softmax_flat(probas, labels, classes="present"):
    """probas (P,C), labels (P,), void pixels already removed."""
    if probas.numel() == 0:
        return probas.sum() * 0.0            # no valid pixel: a zero term
    C = probas.shape[1]
    if C == 1 and not isinstance(classes, str) and len(classes) > 1:
        raise ValueError("Sigmoid output possible only with 1 class")
    losses = []
    which = range(C) if classes in ("all", "present") else classes
    for c in which:
        fg = (labels == c).float()
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, 0 if C == 1 else c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        losses.append(torch.dot(errors_sorted, lovasz_grad(fg[perm]).detach()))
    if not losses:
        return probas.sum() * 0.0            # 'present' with nothing present
    return sum(losses) / len(losses)


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None):
    """probas (B,C,H,W) or one map (B,H,W), labels (B,H,W)."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)

    def flat(p, l):
        Cc = p.shape[1]
        p = p.permute(0, 2, 3, 1).reshape(-1, Cc)
        l = l.reshape(-1)
        if ignore is None:
            return p, l
        keep = l != ignore
        return p[keep], l[keep]
    if per_image:
        vals = [lovasz_softmax_flat(*flat(p.unsqueeze(0), l.unsqueeze(0)), classes=classes) for p, l in zip(probas, labels)]
        return sum(vals) / len(vals)
    return lovasz_softmax_flat(*flat(probas, labels), classes=classes)


def loss_and_grad(probas, labels, classes="present", per_image=False, ignore=None):
    """(loss as a Python float, d loss / d probas) for a plain tensor ``probas``."""
    p = probas.detach().clone().requires_grad_()
    loss = lovasz_softmax(p, labels, classes, per_image, ignore)
    loss.backward()
    return loss.item(), p.grad


def quantised_probas(shape, gen, steps=8):
    """Probabilities with many ties: a softmax rounded to multiples of 1 / steps and renormalised, so that exact 0 and 1
    occur and whole groups of pixels share an error."""
    p = torch.softmax(2.0 * torch.randn(shape, generator=gen), 1)
    q = torch.round(p * steps) / steps
    return q / q.sum(1, keepdim=True)


def one_hot_probas(shape, gen):
    """Saturated probabilities: every error is exactly 0 or 1."""
    B, C, H, W = shape
    return torch.nn.functional.one_hot(torch.randint(0, C, (B, H, W), generator=gen), C).permute(0, 3, 1, 2).float().contiguous()
