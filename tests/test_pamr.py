"""Pixel-adaptive mask refinement without a device: the oracle (tests/pamr_oracle.py, clamped index gathers) against a second
float64 formulation (replicate padding + unfold with a dilation), the oracle's own properties, the host-side geometry check
of the library and the refusal of host tensors."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pamr_oracle as po  # noqa: E402


def replicate_pad(t, p):
    """F.pad(mode="replicate") refuses a pad >= the size: pad in steps (replicating a replicated border is the same clamp)."""
    while p > 0:
        s = min(p, min(t.shape[-2:]) - 1)
        t = F.pad(t, (s, s, s, s), mode="replicate")
        p -= s
    return t


def _pad_by_index(t, p):
    H, W = t.shape[-2:]
    iy = torch.arange(-p, H + p).clamp(0, H - 1)
    ix = torch.arange(-p, W + p).clamp(0, W - 1)
    return t[..., iy, :][..., ix]


def unfold_neighbours(t, dilations):
    """t (B,C,H,W) float64 -> (B,C,8D,H,W) by replicate padding and F.unfold with the dilation; the centre tap dropped."""
    B, C, H, W = t.shape
    out = []
    for d in dilations:
        u = F.unfold(replicate_pad(t, d), kernel_size=3, dilation=d).view(B, C, 9, H, W)
        out.append(torch.cat([u[:, :, :4], u[:, :, 5:]], dim=2))
    return torch.cat(out, dim=2)


def unfold_pamr(images, scores, num_iter, dilations):
    """The formulation a torch user writes (the published one): unfold, torch.std, softmax, a weighted sum per iteration."""
    x, m = images.double(), scores.double()
    D = len(dilations)
    nb = unfold_neighbours(x, dilations)
    samples = torch.cat([nb, x[:, :, None].expand(-1, -1, D, -1, -1)], dim=2)
    sigma = samples.std(dim=2, keepdim=True, unbiased=True)
    a = -(x[:, :, None] - nb).abs() / (1e-8 + 0.1 * sigma)
    w = torch.softmax(a.mean(dim=1), dim=1)
    for _ in range(num_iter):
        m = torch.einsum("bcphw,bphw->bchw", unfold_neighbours(m, dilations), w)
    return w, m


@pytest.mark.parametrize("case", range(len(po.CASES)))
def test_oracle_equals_the_unfold_formulation(case):
    B, H, W, C, K, dil = po.CASES[case]
    img, m = po.make_inputs(B, H, W, C, K, 10 + case)
    w_ref, m_ref = unfold_pamr(img, m, 3, dil)
    w = po.affinity(img, dil)
    assert w.dtype == torch.float64 and tuple(w.shape) == (B, 8 * len(dil), H, W)
    assert (w - w_ref).abs().max().item() < 1e-12
    assert (po.propagate(w, m, 3, dil) - m_ref).abs().max().item() < 1e-12


def test_replicate_padding_in_steps_is_the_clamp():
    t = torch.arange(15.0).view(1, 1, 3, 5)
    for p in (1, 2, 3, 7, 24):
        assert torch.equal(replicate_pad(t, p), _pad_by_index(t, p)), p


def test_oracle_properties():
    B, H, W, C, K, dil = po.CASES[1]
    img, m = po.make_inputs(B, H, W, C, K, 3)
    w = po.affinity(img, dil)
    P = 8 * len(dil)
    assert (w.sum(dim=1) - 1).abs().max().item() < 1e-12 and (w >= 0).all()
    # a flat image: exactly 1 / P
    flat = po.affinity(torch.full((1, 3, 9, 11), 0.37), dil)
    assert torch.equal(flat, torch.full_like(flat, 1.0 / P))
    # a constant score map is a fixed point; no iteration is the identity
    const = torch.full((B, C, H, W), 0.625)
    assert (po.propagate(w, const, 10, dil) - 0.625).abs().max().item() < 1e-13
    assert torch.equal(po.pamr(img, m, 0, dil), m.double())
    # a convex combination stays inside the input's range
    out = po.pamr(img, m, 10, dil)
    assert out.min().item() >= m.min().item() - 1e-12 and out.max().item() <= m.max().item() + 1e-12
    assert out.max().item() - out.min().item() > 0.5          # (and it is not washed out to a constant)


def test_oracle_does_not_depend_on_gain_and_offset():
    """sigma scales with the channel's gain and differences do not see its offset: ImageNet-normalised and raw images give
    the same weights, up to the 1e-8 in the denominator (measured 2.5e-6 at worst)."""
    B, H, W, C, K, dil = po.CASES[1]
    img, m = po.make_inputs(B, H, W, C, K, 5)
    gain = torch.tensor([2.0, 0.5, 4.0]).view(1, 3, 1, 1)
    offset = torch.tensor([-1.0, 0.25, 3.0]).view(1, 3, 1, 1)
    a = po.pamr(img, m, 10, dil)
    b = po.pamr(img.double() * gain.double() + offset.double(), m, 10, dil)
    assert (a - b).abs().max().item() < 1e-5


def test_labels_oracle_and_the_margin_the_device_test_relies_on():
    """Ties pick the lower index, the boundaries are inclusive the documented way, and on the device test's inputs few pixels
    sit within 1e-4 of a decision boundary (the device test may leave out at most 1 %)."""
    s = torch.tensor([0.2, 0.7, 0.7, 0.1]).view(1, 4, 1, 1)
    assert po.labels(s).item() == 1
    assert po.labels(s, min_conf=0.7).item() == 1 and po.labels(s, min_conf=0.7001).item() == 255
    one = torch.tensor([0.5, 0.4999, 0.6]).view(1, 1, 1, 3)
    assert po.labels(one, thresh=0.5).flatten().tolist() == [1, 0, 1]
    for case, (B, H, W, C, K, dil) in enumerate(po.CASES):
        img, m = po.make_inputs(B, H, W, C, K, 10 + case)
        out = po.pamr(img, m, 10, dil)
        close = (po.label_margin(out, 0.3, 0.4) < 1e-4).double().mean().item()
        assert close <= 0.01, (case, close)


def test_workspace_geometry_is_checked_on_the_host():
    from weaklysuperviseddl_amd import ops, _lib
    lib = _lib.lib()
    assert lib.wsdl_pamr_workspace(16, 2, 256, 256, 6) >= 2 * 16 * 2 * 256 * 256 * 4
    assert ops.pamr_workspace(16, 3, 2, 256, 256) == lib.wsdl_pamr_workspace(16, 2, 256, 256, 6)
    assert lib.wsdl_pamr_workspace(1, 33, 8, 8, 6) == 0          # C = 33
    assert lib.wsdl_pamr_workspace(1, 2, 8, 8, 9) == 0           # D = 9
    assert lib.wsdl_pamr_workspace(1, 2, 0, 8, 6) == 0           # H = 0
    assert lib.wsdl_pamr_workspace(0, 2, 8, 8, 6) == 0 and lib.wsdl_pamr_workspace(1, 0, 8, 8, 6) == 0
    assert ops.pamr_workspace(1, 5, 2, 8, 8) == 0                # K = 5
    assert ops.pamr_workspace(1, 3, 33, 8, 8) == 0
    assert ops.pamr_workspace(1, 3, 2, 8, 8, (1,) * 9) == 0
    assert ops.pamr_workspace(1, 3, 2, 8, 8, (1, 65)) == 0       # d = 65
    assert ops.pamr_workspace(1, 3, 2, 8, 8, (0,)) == 0 and ops.pamr_workspace(1, 3, 2, 8, 8, ()) == 0
    assert ops.pamr_workspace(1, 3, 2, 0, 8) == 0
    assert ops.pamr_workspace(1, 4, 32, 8, 8, (64,) * 8) > 0     # the limits themselves are inside
    # the entry points refuse the same geometry before anything is launched (no device here)
    import ctypes as C
    dil = (C.c_int * 2)(1, 65)
    assert lib.wsdl_pamr_affinity(8, 1, 3, 8, 8, dil, 2, 8, None) != 0 and b"dilations" in lib.wsdl_last_error()
    dil = (C.c_int * 1)(1)
    assert lib.wsdl_pamr_affinity(8, 1, 5, 8, 8, dil, 1, 8, None) != 0
    assert lib.wsdl_pamr_propagate(8, 64, 64, 1, 2, 4, 4, dil, 1, 3, 8, 1 << 20, None) != 0 and b"overlap" in lib.wsdl_last_error()
    assert lib.wsdl_pamr_propagate(8, 64, 4096, 1, 2, 4, 4, dil, 1, -1, 8, 1 << 20, None) != 0


def test_host_tensors_and_bad_options_are_refused():
    from weaklysuperviseddl_amd import ops, nn as wnn
    x, m = torch.rand(1, 3, 8, 8), torch.rand(1, 2, 8, 8)
    with pytest.raises(ops.WsdlError):
        ops.pamr_affinity(x)
    with pytest.raises(ops.WsdlError):
        ops.pamr(x, m)
    with pytest.raises(ops.WsdlError):
        ops.pamr_labels(m)
    with pytest.raises(ops.WsdlError):
        wnn.PAMR()(x, m)
    for kw in (dict(num_iter=-1), dict(num_iter=1.5), dict(dilations=(0,)), dict(dilations=(1, 65)), dict(dilations=(1,) * 9),
               dict(dilations=()), dict(dilations=(1.0,))):
        with pytest.raises(ValueError):
            ops.pamr(x, m, **kw)
        with pytest.raises(ValueError):
            wnn.PAMR(**kw)
    assert wnn.PAMR().num_iter == 10 and wnn.PAMR().dilations == (1, 2, 4, 8, 12, 24) == ops.PAMR_DILATIONS == po.DILATIONS
    assert "num_iter=10" in repr(wnn.PAMR())


def test_callers_keep_their_defaults():
    import inspect
    from weaklysuperviseddl_amd.TraditionalModel import refine_dataset, generate_pseudo_masks
    p = inspect.signature(refine_dataset).parameters
    assert p["method"].default == "ncut" and p["pamr_kwargs"].default is None and p["repeats"].default == 5
    assert inspect.signature(generate_pseudo_masks).parameters["pamr"].default is None
    with pytest.raises(ValueError):
        refine_dataset(None, [], method="crf")
