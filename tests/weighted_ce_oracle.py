"""float64 restatement of the weighted cross entropy (ops.cross_entropy with its options): loss and closed-form gradient.

For pixel i with label y, v = [y != ignore_index], softmax s over the C planes, class weights w (default 1), pixel weight p
(default 1) and smoothing e:

    l_i = v p [ (1-e) w[y] (-log s[y]) + (e/C) sum_c w[c] (-log s[c]) ]
    'none': l;  'sum': sum_i l_i;  'mean': sum_i l_i / sum_i v p w[y_i]
    dl_i/dz[c] = v p [ s[c] A - (1-e) w[y] [c = y] - (e/C) w[c] ],  A = (1-e) w[y] + (e/C) sum_c w[c]

A pixel with p == 0 is an ignored pixel.  tests/test_weighted_ce.py pins this against torch.nn.functional.cross_entropy.
"""
import torch


def weighted_ce(logits, labels, ignore_index=-100, weight=None, label_smoothing=0.0, reduction="mean", pixel_weight=None,
                upstream=None):
    """(loss, dlogits) in float64 on the CPU.  logits (B,C,H,W), labels (B,H,W) int64 - every label ignore_index or in [0,C);
    ``upstream``: the gradient arriving at the loss - a scalar for 'mean' / 'sum', (B,H,W) for 'none' (default ones)."""
    z = logits.detach().cpu().double()
    y = labels.detach().cpu().long()
    B, C, H, W = z.shape
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().cpu().double()
    p = torch.ones(B, H, W, dtype=torch.float64) if pixel_weight is None else pixel_weight.detach().cpu().double()
    e = float(label_smoothing)
    v = ((y != ignore_index) & (p != 0)).double()
    ys = torch.where(v.bool(), y, torch.zeros_like(y))
    logs = torch.log_softmax(z, dim=1)
    s = logs.exp()
    wy = w[ys]
    nll = -logs.gather(1, ys[:, None]).squeeze(1)
    wv = w.view(1, C, 1, 1)
    smooth = -(wv * logs).sum(1)
    pix = v * p * ((1 - e) * wy * nll + (e / C) * smooth)
    A = (1 - e) * wy + (e / C) * w.sum()
    onehot = torch.zeros_like(z).scatter_(1, ys[:, None], 1.0)
    grad = (v * p)[:, None] * (s * A[:, None] - (1 - e) * wy[:, None] * onehot - (e / C) * wv)
    if reduction == "none":
        g = torch.ones(B, H, W, dtype=torch.float64) if upstream is None else upstream.detach().cpu().double()
        return pix, grad * g[:, None]
    g = 1.0 if upstream is None else float(upstream)
    if reduction == "sum":
        return pix.sum(), grad * g
    if reduction == "mean":
        den = (v * p * wy).sum()
        return pix.sum() / den, grad * (g / den)
    raise ValueError(reduction)
