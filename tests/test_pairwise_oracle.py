"""The torch oracle of the pairwise-affinity losses (oracle/losses.py) in float64 against the per-pixel numpy loop of
tests/pairwise_oracle.py: two formulations that share no code (``F.pad`` and stacked views there, explicit reflect indices
here) must agree to 1e-12 relative - loss, every affinity, the forward-half table of the affinity cache - and the oracle's
autograd gradient must be the loop's central difference.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairwise_oracle as po  # noqa: E402

CASES = ((1, 1, 2, 2, 3), (1, 2, 3, 3, 5), (1, 2, 4, 4, 7), (2, 3, 5, 9, 5), (1, 2, 9, 13, 5), (1, 3, 7, 4, 7))
REL = 1e-12


def inputs(B, C, H, W, seed, softmax):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64)
    preds = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2
    return image, (preds if softmax else torch.rand(B, C, H, W, generator=g, dtype=torch.float64))


def close(got, want, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= rel * np.abs(want)).all())


@pytest.mark.parametrize("space", (None, 0.0, 1.5), ids=("none", "zero", "space"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:4])) + f"w{c[4]}")
def test_loss_and_affinities_equal_the_loop(case, space):
    import oracle
    from oracle.losses import _affinity_stack
    B, C, H, W, window = case
    K = window * window - 1
    for softmax, norm in ((True, 0), (False, 1), (True, 1), (False, 0)):
        image, preds = inputs(B, C, H, W, 11 * H + W, softmax)
        ref = oracle.pairwise_affinity_loss(preds, image, window, 0.3, space, softmax, norm)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == ((B,) if norm else ())
        mine = po.loss(preds, image, window, 0.3, space, softmax, norm)
        assert close(ref.numpy(), mine), (softmax, norm, ref, mine)
        assert (C == 1 and softmax) == (not np.any(mine))          # one class under a softmax: P == 1, nothing to compare
    stack = _affinity_stack(image, window, 0.3, space)
    loop = po.affinities(image, window, 0.3, space)
    assert tuple(stack.shape) == (K, B, H, W) == loop.shape and stack.dtype == torch.float64
    assert close(stack.numpy(), loop)
    maps = oracle.compute_affinities(image, 0.3, space, window)
    assert len(maps) == K and tuple(maps[0].shape) == (B, 1, H, W)
    assert close(torch.stack(maps)[:, :, 0].numpy(), loop)
    single = oracle.ConstrainToBoundaryLossSingle.compute_affinities_single(image[0], 0.3, space, window)
    assert len(single) == K and tuple(single[0].shape) == (1, H, W) and close(torch.stack(single)[:, 0].numpy(), loop[:, 0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:4])) + f"w{c[4]}")
def test_forward_half_table_of_the_cache(case):
    """K/2 maps, (dy == 0, dx > 0) then dy > 0 in raster order, 0 at partners outside the image: the loop against the table
    cut out of the torch oracle's stack, and against the full stack's mirrored half (the affinity is symmetric)."""
    from oracle.losses import _affinity_stack
    B, _, H, W, window = case
    image, _ = inputs(B, 1, H, W, 5 * H + W, True)
    offs = po.forward_offsets(window)
    R = window // 2
    assert len(offs) == (window * window - 1) // 2 and offs[0] == (0, 1) and offs[R] == (1, -R) and offs[-1] == (R, R)
    table = po.forward_half_cache(image, window, 0.3)
    stack = _affinity_stack(image, window, 0.3, None)
    cut = po.forward_half_of_stack(stack, window).numpy()
    assert table.shape == (len(offs), B, H, W) == cut.shape
    assert np.array_equal(table == 0, cut == 0) and close(cut, table)
    full = po.offsets(window)
    for k, (dy, dx) in enumerate(offs):
        back = stack[full.index((-dy, -dx))].numpy()
        for y in range(H):
            for x in range(W):
                inside = 0 <= y + dy < H and 0 <= x + dx < W
                assert (table[k, :, y, x] > 0).all() == inside
                if inside:       # the partner's backward entry is this pixel's forward entry
                    assert close(back[:, y + dy, x + dx], table[k, :, y, x])


@pytest.mark.parametrize("case", ((1, 2, 3, 3, 5), (1, 3, 5, 9, 5)), ids=("1x2x3x3", "1x3x5x9"))
@pytest.mark.parametrize("softmax,norm,space", ((True, 0, None), (False, 1, 1.5)), ids=("ncut", "boundary"))
def test_autograd_gradient_equals_central_differences_of_the_loop(case, softmax, norm, space):
    import oracle
    B, C, H, W, window = case
    image, preds = inputs(B, C, H, W, 3 * H + W, softmax)
    weights = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    p = preds.clone().requires_grad_()
    out = oracle.pairwise_affinity_loss(p, image, window, 0.3, space, softmax, norm)
    (out * weights).sum().backward() if norm else out.backward()
    fd = po.central_difference_gradient(preds, image, window, 0.3, space, softmax, norm, weights if norm else None, h=1e-6)
    err = np.abs(fd - p.grad.numpy()).max()
    assert p.grad.abs().max().item() > 0 and err <= 1e-7 * p.grad.abs().max().item(), (err, p.grad.abs().max().item())


@pytest.mark.parametrize("window", (3, 5, 7))
def test_closed_forms_on_the_oracle(window):
    """A flat image: every affinity is exp(-|o|^2 / (2 ss^2)), exactly 1 without the spatial term.  Logits equal at every
    pixel: the loss is 0 (under ATen's softmax: at most the square of an ulp)."""
    import oracle
    from oracle.losses import _affinity_stack
    H, W = window // 2 + 1, 2 * window + 1
    flat = torch.full((2, 3, H, W), 0.375, dtype=torch.float64)
    for space in (None, 0.0):
        assert torch.equal(_affinity_stack(flat, window, 0.05, space), torch.ones(window * window - 1, 2, H, W, dtype=torch.float64))
    want = torch.tensor([math.exp(-(dy * dy + dx * dx) / (2 * 1.5 ** 2)) for dy, dx in po.offsets(window)], dtype=torch.float64)
    got = _affinity_stack(flat, window, 0.05, 1.5)
    assert close(got.numpy(), want.view(-1, 1, 1, 1).expand_as(got).numpy())
    image, _ = inputs(2, 3, H, W, 7, True)
    same = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64).view(1, 3, 1, 1).expand(2, 3, H, W).contiguous()
    for softmax, norm in ((True, 0), (False, 1), (True, 1), (False, 0)):
        # without the softmax every difference is exactly 0; ATen's softmax runs a vector body and a scalar tail whose exp may
        # differ in the last place, so equal logits give probabilities equal to one ulp of 1 (2^-52) and a loss - a weighted
        # mean of squared differences, weights <= 1 - of at most (2^-52)^2
        tiny = (2.0 ** -52) ** 2 if softmax else 0.0
        out = oracle.pairwise_affinity_loss(same, image, window, 0.1, 1.5, softmax, norm)
        assert (out >= 0).all() and out.max().item() <= tiny
        assert np.min(po.loss(same, image, window, 0.1, 1.5, softmax, norm)) >= 0
        assert np.max(po.loss(same, image, window, 0.1, 1.5, softmax, norm)) <= tiny
