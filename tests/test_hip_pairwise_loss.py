"""The pairwise-affinity losses on the device - ``pairwise_kernel<R, CACHED>``, ``pairwise_cache_kernel``, ``affinities_kernel``
and ``finalize_sum_kernel`` of csrc/resample_loss.hip behind ``ops.pairwise_affinity_loss``, ``ops.pairwise_cache``,
``ops.compute_affinities``, ``LocalNormalizedCutLoss`` and ``ConstrainToBoundaryLossSingle`` - against the float64 oracle
(oracle/losses.py, itself held to the per-pixel loop of tests/pairwise_oracle.py by tests/test_pairwise_oracle.py), at the
borders, partial tiles, class counts and image contents where the kernel takes another path.

Every case builds its inputs once in float32; the float64 oracle and its autograd gradient are taken from those same values
cast up, the yardstick is the SAME oracle run in torch float32 on the CPU: ``yard = max |float32 oracle - float64|``, per
case, never taken from the device.  The error of the device is the max-norm ``max |device - float64|`` over the whole tensor.

  * gradient bound: the project's standing one, ``max(4 x yard, 2^-23 max |float64 gradient|)`` (plus, where there is a
    spatial term, the derived term below).
  * loss bound: ``4 x yard + (window^2 C + 16) 2^-24 |loss|``.  Torch sums the oracle pairwise, so its float32 loss sits
    at about an ulp of float64 and the yardstick alone says little about a sequential sum.  A kernel thread adds its
    window^2 C terms, all >= 0, in ONE float32 fmaf chain: at worst (chain depth) x 2^-24 of the sum; the block tree adds 8
    + 4 levels (the 16), the tile partials are added in double.

  * one derived term on the gradient, only where ``sigma_space > 0`` (``spatial_weight_term``): without it the device read
    1.03 x its bound at 1x2x9x33, window 7, probabilities, sigma_space 5 (4.61e-10 against 4.48e-10 at a gradient maximum of
    1.2e-3; every other case passed).  The oracle takes ONE exp of the summed colour and spatial exponents per pair; the
    kernel folds reflect padding into per-axis pair weights, so its weight of a pair is ``(wyF wxF + wyR wxR) cc`` with
    every factor rounded on its way.  Per factor, in units of 2^-24 relative: ``g1[d] = expf(-d^2 inv2ss)``, one per axis,
    2 each (expf is good to an ulp) plus 4 |x| each for its argument (``2 ss^2``, its reciprocal and the product with d^2:
    four roundings, |x| <= R^2 / (2 ss^2)); a border pixel adds up to three ``g1`` per axis (2 additions, 2 each); the
    product of the two axes 1; ``wf + wr`` 1; the product with the colour affinity 1: 11 + 8 R^2 / (2 ss^2) in all.  The
    error is relative to each pair's term, so pixel by pixel the gradient may move by that many 2^-24 of the sum of its
    pairs' ABSOLUTE terms ``S = 2 / N sum_pairs a |dP|`` (times the upstream weight; through the softmax's Jacobian where
    there is one), taken from the float64 oracle - never from the device.  Without the spatial term every ``g1`` is 1,
    the per-axis weights are small integers and the term is 0: those cases keep the standing bound alone.

A missing or doubled pair moves the gradient at its pixel by about 1 / K of its value, orders of magnitude above either bound
(the derived term is at most 12.4 x 2^-24 of S at sigma_space 5 and 75 x 2^-24 at sigma_space 0.5).  The worst
device-error-to-bound ratios, reported with ``report_line`` per case and per family, stand in README.md."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairwise_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---- the table: (family, B, C, H, W, window, sigma_color, sigma_space, softmax, normalise, image, preds) ---------------------
NCUT = (0.0, True, 0)                  # sigma_space, softmax, normalise: LocalNormalizedCutLoss
BOUNDARY = (5.0, False, 1)             # ConstrainToBoundaryLossSingle: probabilities in, one loss per image, colour + space

GEOMETRY = ((1, 2, 2, 2, 3), (1, 2, 3, 3, 5), (1, 2, 4, 4, 7),          # the minimum side R + 1
            (2, 3, 5, 9, 5),                                           # H in (2R, 4R]: no inner row
            (1, 2, 9, 13, 5), (1, 2, 13, 13, 7),                       # exactly one inner row
            (2, 2, 8, 32, 5),                                          # exactly one full tile
            (1, 2, 9, 33, 3), (1, 2, 9, 33, 5), (1, 2, 9, 33, 7),      # a second tile row and column with a single active line
            (1, 3, 17, 70, 7),                                         # three ragged column tiles
            (1, 2, 300, 3, 5), (1, 2, 3, 300, 5),                      # 38 tiles of width R + 1; H = R + 1
            (3, 2, 16, 64, 5))                                         # B = 3: per-image losses
CLASSES = tuple((2, C, 9, 33, 5) for C in (1, 7, 8, 9, 16, 17, 21, 32)) + tuple((2, C, 9, 33, 7) for C in (8, 9, 27))
CONTENT_SHAPE = (2, 3, 17, 40, 5)

CASES = tuple(("geometry",) + g + (0.1,) + mode + ("smooth", "random") for g in GEOMETRY for mode in (NCUT, BOUNDARY))
CASES += tuple(("classes",) + c + (0.1,) + mode + ("smooth", "random") for c in CLASSES for mode in (NCUT, BOUNDARY))
CASES += tuple(("contents",) + CONTENT_SHAPE + (sc, ss, True, 0, image, preds) for sc, ss, image, preds in (
    (0.1, 0.0, "noise", "random"), (0.5, 0.5, "noise", "random"), (0.1, 0.0, "flat", "random"), (0.1, 0.0, "step", "random"),
    (0.1, 0.0, "imagenet", "random"), (0.1, 0.0, "smooth", "saturated"), (0.1, 0.0, "smooth", "equal"),
    (0.05, 0.0, "smooth", "random"), (1.0, 0.0, "smooth", "random")))
MODULE_CASES = (("modules", 1, 21, 9, 33, 5, 0.05, 0.0, True, 0, "smooth", "random"),
                ("modules", 2, 21, 9, 33, 5, 0.05, 0.0, True, 0, "smooth", "random"),
                ("modules", 1, 21, 9, 33, 5, 0.1, 5.0, False, 1, "smooth", "random"),
                ("modules", 2, 21, 9, 33, 5, 0.1, 5.0, False, 1, "smooth", "random"))


def name_of(case):
    fam, B, C, H, W, window, sc, ss, softmax, norm, image, preds = case
    return (f"{B}x{C}x{H}x{W} w{window} sc={sc:g} ss={ss:g} {'softmax' if softmax else 'probs'} norm={norm}"
            + ("" if image == "smooth" else f" {image}") + ("" if preds == "random" else f" {preds}"))


def is_exactly_zero(case):
    """One class under a softmax (P == 1) and logits equal at every pixel: every difference is exactly 0."""
    return (case[2] == 1 and case[8]) or case[11] == "equal"


def make_image(kind, B, H, W, seed):
    from conftest import smooth_image
    if kind == "noise":
        return po.noise_image(B, H, W, seed)
    if kind == "flat":
        return po.flat_image(B, H, W)
    if kind == "step":
        return po.step_image(B, H, W)
    img = smooth_image(B, H, W, seed)
    return ((img - 0.45) / 0.225).contiguous() if kind == "imagenet" else img


def make_preds(kind, B, C, H, W, softmax, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":
        return (torch.randn(1, C, 1, 1, generator=g) * 2).expand(B, C, H, W).contiguous()
    logits = torch.randn(B, C, H, W, generator=g) * (60.0 if kind == "saturated" else 2.0)
    if softmax:
        return logits
    return torch.rand(B, C, H, W, generator=g) if C == 1 else F.softmax(logits, 1)


def upstream(B, norm, dtype=torch.float32):
    """The incoming gradient: one weight per image where the loss is per image (the scaling in the op's backward)."""
    return torch.linspace(0.5, 1.5, B).to(dtype) if norm else None


def run_oracle(preds, image, case, dtype):
    import oracle
    _, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    p = preds.detach().to(dtype).clone().requires_grad_()
    out = oracle.pairwise_affinity_loss(p, image.to(dtype), window, sc, ss, softmax, norm)
    (out * upstream(B, norm, dtype)).sum().backward() if norm else out.backward()
    assert out.dtype == dtype and p.grad.dtype == dtype
    return out.detach().reshape(-1), p.grad


def spatial_weight_term(preds, image, case):
    """The derived term of the gradient bound (module docstring), element by element in float64: ``(11 + 8 R^2 / (2 ss^2))
    2^-24 S`` with ``S(q, c) = w_b 2 / N sum a |P_c(q) - P_c(p)|`` over every pair the pixel takes part in, as source or as
    (reflected) partner; under the softmax ``P_c (S_c + sum_c' P_c' S_c')``.  0 without a spatial term."""
    from oracle.losses import _affinity_stack, _shifted_stack
    _, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    if not ss > 0:
        return torch.zeros(B, C, H, W, dtype=torch.float64)
    P = preds.detach().double()
    P = F.softmax(P, 1) if softmax else P
    a = _affinity_stack(image.double(), window, sc, ss)
    d = (P.unsqueeze(0) - _shifted_stack(P, window)).abs()
    u = torch.zeros_like(P).requires_grad_()          # d / du of sum a |dP| (u(q) + u(p)): the pairs' weights, gathered at both ends
    (a.unsqueeze(2) * d * (u.unsqueeze(0) + _shifted_stack(u, window))).sum().backward()
    K = window * window - 1
    S = u.grad * (2.0 / (H * W * K if norm else B * H * W * K * C))
    if norm:
        S = S * upstream(B, norm, torch.float64).view(B, 1, 1, 1)
    if softmax:
        S = P * (S + (P * S).sum(dim=1, keepdim=True))
    R = window // 2
    return (11.0 + 8.0 * R * R / (2.0 * ss * ss)) * 2.0 ** -24 * S


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs (float32), the float64 oracle with its autograd gradient and the float32 yardsticks of one case - computed once,
    shared, never written."""
    fam, B, C, H, W, window, sc, ss, softmax, norm, image_kind, preds_kind = case
    seed = 1000 * window + 10 * H + W + C
    image = make_image(image_kind, B, H, W, seed)
    preds = make_preds(preds_kind, B, C, H, W, softmax, seed + 1)
    assert image.dtype == torch.float32 and preds.dtype == torch.float32
    L64, g64 = run_oracle(preds, image, case, torch.float64)
    L32, g32 = run_oracle(preds, image, case, torch.float32)
    assert not preds.requires_grad and preds.grad is None
    return dict(image=image, preds=preds, L64=L64, g64=g64, yard_L=(L32.double() - L64).abs().max().item(),
                yard_g=(g32.double() - g64).abs().max().item(), term_g=spatial_weight_term(preds, image, case))


def loss_ratio(L, r, case):
    """max over the images of |device - float64| / (4 yard + (window^2 C + 16) 2^-24 |loss|); 0 / 0 counts as 0."""
    depth = case[5] * case[5] * case[2] + 16
    err = (L.detach().cpu().double().reshape(-1) - r["L64"]).abs()
    bnd = 4.0 * r["yard_L"] + depth * 2.0 ** -24 * r["L64"].abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bnd).max().item()


def grad_ratio(g, r):
    """max over the elements of |device - float64| / (max(4 yard, 2^-23 max |gradient|) + the derived term there)."""
    err = (g.detach().cpu().double() - r["g64"]).abs()
    bnd = max(4.0 * r["yard_g"], ULP * r["g64"].abs().max().item()) + r["term_g"]
    return torch.where(err == 0, torch.zeros_like(err), err / bnd).max().item()


def device_loss(case, preds, image, cache=None):
    from weaklysuperviseddl_amd import ops
    _, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    return ops.pairwise_affinity_loss(preds, image, window, sc, ss, softmax, norm, cache=cache)


def loss_and_gradient(case, preds, image, cache=None):
    p = preds.clone().requires_grad_()
    L = device_loss(case, p, image, cache)
    (L * upstream(case[1], case[9]).to(L.device)).sum().backward() if case[9] else L.backward()
    return L.detach(), p.grad


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_per_family():
    yield
    from conftest import report_line
    for fam, (rl, rg) in WORST.items():
        report_line(f"pairwise {fam}: worst device error / bound: loss {rl:.2f}, gradient {rg:.2f}")


def record(case, rl, rg):
    from conftest import report_line
    fam = case[0]
    WORST[fam] = (max(WORST.get(fam, (0, 0))[0], rl), max(WORST.get(fam, (0, 0))[1], rg))
    report_line(f"pairwise {fam} {name_of(case)}: device error / bound: loss {rl:.2f}, gradient {rg:.2f}")


@pytest.mark.parametrize("case", CASES, ids=name_of)
def test_loss_and_gradient_against_float64(dev, case):
    from weaklysuperviseddl_amd import ops
    fam, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    r = reference(case)
    image, preds = r["image"].to(dev), r["preds"].to(dev)
    L, g = loss_and_gradient(case, preds, image)
    rl, rg = loss_ratio(L, r, case), grad_ratio(g, r)
    record(case, rl, rg)
    print(f"{name_of(case)}: loss {L.reshape(-1).tolist()} float64 {r['L64'].tolist()} yard {r['yard_L']:.3e} ratio {rl:.3f}; "
          f"gradient max {r['g64'].abs().max().item():.3e} yard {r['yard_g']:.3e} derived term at most {r['term_g'].max().item():.3e} ratio {rg:.3f}")
    assert L.dtype == torch.float32 and tuple(L.shape) == ((B,) if norm else ()) and tuple(g.shape) == (B, C, H, W)
    assert torch.isfinite(L).all() and torch.isfinite(g).all()
    if is_exactly_zero(case):
        # float64's own value: 0, or the (2^-52)^2 that ATen's softmax leaves between equal pixels (tests/test_pairwise_oracle.py)
        assert r["L64"].abs().max().item() <= (2.0 ** -52) ** 2 and r["g64"].abs().max().item() <= 2.0 ** -52
        assert not L.any() and not g.any()
    else:
        assert r["L64"].min().item() > 0 and r["g64"].abs().max().item() > 0
        assert rl <= 1.0, (rl, r["yard_L"])
        assert rg <= 1.0, (rg, r["yard_g"])
    # the cached variant, a second call and the launch without a gradient buffer: the same bits; the inputs are never written
    cache = ops.pairwise_cache(image, window, sc)
    Lc, gc = loss_and_gradient(case, preds, image, cache)
    assert torch.equal(Lc, L) and torch.equal(gc, g)
    L2, g2 = loss_and_gradient(case, preds, image)
    assert torch.equal(L2, L) and torch.equal(g2, g)
    assert not preds.requires_grad
    Ln = device_loss(case, preds, image)
    assert not Ln.requires_grad and torch.equal(Ln, L) and torch.equal(device_loss(case, preds, image, cache), L)
    assert torch.equal(preds.cpu(), r["preds"]) and torch.equal(image.cpu(), r["image"])


@pytest.mark.parametrize("case", (("symmetry", 2, 3, 5, 9, 5, 0.1) + NCUT + ("smooth", "random"),
                                  ("symmetry", 2, 3, 5, 9, 5, 0.1) + BOUNDARY + ("smooth", "random"),
                                  ("symmetry", 1, 2, 9, 33, 7, 0.1) + NCUT + ("smooth", "random"),
                                  ("symmetry", 1, 2, 9, 33, 7, 0.1) + BOUNDARY + ("smooth", "random")), ids=name_of)
def test_mirror_symmetry_where_every_pixel_is_a_border_pixel(dev, case):
    """Reflect padding commutes with a flip: image and predictions flipped along W, H or both give the float64 loss, and the
    gradient flipped back is the float64 gradient, each under its bound."""
    r = reference(case)
    for dims in ((-1,), (-2,), (-2, -1)):
        L, g = loss_and_gradient(case, r["preds"].flip(dims).contiguous().to(dev), r["image"].flip(dims).contiguous().to(dev))
        rl, rg = loss_ratio(L, r, case), grad_ratio(g.flip(dims), r)
        record(case[:11] + ("flipped along " + "".join("HW"[d + 2] for d in dims),), rl, rg)
        assert rl <= 1.0, (dims, rl)
        assert rg <= 1.0, (dims, rg)


@pytest.mark.parametrize("kind", ("smooth", "noise"))
@pytest.mark.parametrize("shape,window", (((1, 2, 2), 3), ((1, 4, 4), 7), ((2, 9, 33), 5), ((2, 17, 40), 7)),
                         ids=("1x3x2x2w3", "1x3x4x4w7", "2x3x9x33w5", "2x3x17x40w7"))
def test_cache_against_the_loop(dev, shape, window, kind):
    """``ops.pairwise_cache``: K/2 maps, (dy == 0, dx > 0) then dy > 0 in raster order, exactly 0.0 where the partner is outside
    the image, the pair's colour affinity elsewhere."""
    from conftest import report_line
    from oracle.losses import _affinity_stack
    from weaklysuperviseddl_amd import ops
    (B, H, W), sc = shape, 0.1
    image = make_image(kind, B, H, W, 31 * H + W)
    want = torch.from_numpy(po.forward_half_cache(image, window, sc))
    y32 = po.forward_half_of_stack(_affinity_stack(image, window, sc, None), window)
    assert y32.dtype == torch.float32
    yard = (y32.double() - want).abs().max().item()
    got = ops.pairwise_cache(image.to(dev), window, sc)
    assert tuple(got.shape) == ((window * window - 1) // 2, B, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    outside = torch.from_numpy(po.forward_half_cache(torch.zeros_like(image), window, sc)) == 0   # (a flat image: 1 inside)
    assert torch.equal(got.cpu()[outside], torch.zeros(int(outside.sum())))
    assert (got.cpu()[~outside] > 0).all() or kind == "noise"
    err, bnd = (got.cpu().double() - want).abs().max().item(), max(4.0 * yard, ULP)
    report_line(f"pairwise cache {B}x3x{H}x{W} w{window} {kind}: device error / bound {err / bnd:.2f}")
    assert err <= bnd, (err, bnd)
    assert torch.equal(ops.pairwise_cache(image.to(dev), window, sc), got)


@pytest.mark.parametrize("kind", ("smooth", "noise"))
@pytest.mark.parametrize("shape,window", (((1, 2, 2), 3), ((1, 4, 4), 7), ((2, 9, 33), 3), ((2, 9, 33), 5), ((2, 9, 33), 7),
                                          ((3, 17, 40), 3), ((3, 17, 40), 5), ((3, 17, 40), 7)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"w{v}")
def test_compute_affinities_against_float64(dev, shape, window, kind):
    """The K maps of ``compute_affinities`` in dy-major order, shape (K, B, 1, H, W), and ``compute_affinities_single``, with
    and without the spatial term, under ``max(4 x yard, 2^-23 max |value|)``."""
    from conftest import report_line
    from oracle.losses import _affinity_stack
    from weaklysuperviseddl_amd import ops
    from weaklysuperviseddl_amd.TraditionalModel import ConstrainToBoundaryLossSingle, compute_affinities
    B, H, W = shape
    K = window * window - 1
    image = make_image(kind, B, H, W, 17 * H + W)
    worst = 0.0
    for space in (0, None, 0.5, 5):
        a64 = _affinity_stack(image.double(), window, 0.1, space)
        yard = (_affinity_stack(image, window, 0.1, space).double() - a64).abs().max().item()
        bnd = max(4.0 * yard, ULP * a64.abs().max().item())
        got = ops.compute_affinities(image.to(dev), 0.1, space, window)
        assert tuple(got.shape) == (K, B, 1, H, W) and got.dtype == torch.float32
        err = (got.cpu().double()[:, :, 0] - a64).abs().max().item()
        worst = max(worst, err / bnd)
        assert err <= bnd, (space, err, bnd)
        maps = compute_affinities(image.to(dev), 0.1, space, window)
        assert len(maps) == K and all(torch.equal(m, got[k]) for k, m in enumerate(maps))
        single = ConstrainToBoundaryLossSingle.compute_affinities_single(image[B - 1].to(dev), 0.1, space, window)
        assert len(single) == K and tuple(single[0].shape) == (1, H, W)
        assert (torch.stack(single).cpu().double()[:, 0] - a64[:, B - 1]).abs().max().item() <= bnd
        if not space:            # the two spellings of "no spatial term": the same bits
            assert torch.equal(got, ops.compute_affinities(image.to(dev), 0.1, 0.0, window))
    report_line(f"pairwise affinities {B}x3x{H}x{W} w{window} {kind}: worst device error / bound {worst:.2f}")


@pytest.mark.parametrize("case", MODULE_CASES, ids=name_of)
def test_modules_at_21_classes(dev, case):
    """``LocalNormalizedCutLoss`` and ``ConstrainToBoundaryLossSingle`` on a (C,H,W) input (the B = 1 cases) and on a batch."""
    from weaklysuperviseddl_amd.TraditionalModel import ConstrainToBoundaryLossSingle, LocalNormalizedCutLoss
    _, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    r = reference(case)
    crit = LocalNormalizedCutLoss() if softmax else ConstrainToBoundaryLossSingle()
    assert (crit.sigma_color, crit.window_size) == (sc, window) and (softmax or crit.sigma_space == ss)
    image, p = r["image"].to(dev), r["preds"].to(dev).requires_grad_()
    L = crit(p[0], image[0]) if B == 1 else crit(p, image)
    assert tuple(L.shape) == ((B,) if norm and B > 1 else ())
    (L * upstream(B, norm).to(dev)).sum().backward() if norm else L.backward()
    rl, rg = loss_ratio(L, r, case), grad_ratio(p.grad, r)
    record(case, rl, rg)
    assert rl <= 1.0, (rl, r["yard_L"])
    assert rg <= 1.0, (rg, r["yard_g"])
    Lo, go = loss_and_gradient(case, r["preds"].to(dev), image)
    assert torch.equal(Lo.reshape(-1), L.detach().reshape(-1)) and torch.equal(go, p.grad)


@pytest.mark.parametrize("case", MODULE_CASES[1::2], ids=name_of)
def test_strided_inputs_give_the_bits_of_their_dense_copies(dev, case):
    """A channel slice of a wider tensor, a permuted NHWC tensor and a strided image: the ops work on a dense copy, the loss
    and the gradient are those of ``.contiguous()``, and the gradient arrives at the strided leaf."""
    _, B, C, H, W, window, sc, ss, softmax, norm, _, _ = case
    r = reference(case)
    image, preds = r["image"].to(dev), r["preds"].to(dev)
    L0, g0 = loss_and_gradient(case, preds, image)
    w = upstream(B, norm).to(dev) if norm else torch.ones((), device=dev)

    wide = torch.cat([preds[:, :1] + 1, preds, preds[:, :1] - 1], dim=1).requires_grad_()
    view = wide[:, 1:1 + C]
    assert not view.is_contiguous()
    L = device_loss(case, view, image)
    (L * w).sum().backward()
    assert torch.equal(L.detach(), L0) and torch.equal(wide.grad[:, 1:1 + C], g0)
    assert not wide.grad[:, 0].any() and not wide.grad[:, -1].any()

    nhwc = preds.permute(0, 2, 3, 1).contiguous().requires_grad_()
    view = nhwc.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    L = device_loss(case, view, image)
    (L * w).sum().backward()
    assert torch.equal(L.detach(), L0) and torch.equal(nhwc.grad.permute(0, 3, 1, 2), g0)

    strided = torch.cat([image[:, :1], image, image[:, :1]], dim=1)[:, 1:4]
    assert not strided.is_contiguous()
    L, g = loss_and_gradient(case, preds, strided)
    assert torch.equal(L, L0) and torch.equal(g, g0)
    Lv = device_loss(case, wide.detach()[:, 1:1 + C], strided)        # the launch without a gradient buffer
    assert torch.equal(Lv, L0)


def test_refusals_name_their_cause(dev):
    """What the ABI does not accept raises ``ops.WsdlError`` and leaves the cause in ``wsdl_last_error``; the accepted neighbours
    (C = 27 at window 7, C = 32 at window 5, a side of R + 1) are launched by the cases above.  A refusal leaves no trace:
    the call after it computes what it computed before."""
    from weaklysuperviseddl_amd import lib, ops
    from conftest import smooth_image

    def refused(call, cause, in_library=True):
        with pytest.raises(ops.WsdlError) as e:
            call()
        assert cause in str(e.value), (cause, str(e.value))
        if in_library:
            assert cause in lib().wsdl_last_error().decode(), (cause, lib().wsdl_last_error().decode())

    def inputs(B, C, H, W):
        return torch.rand(B, C, H, W, device=dev).requires_grad_(), smooth_image(B, H, W, 3).to(dev)
    p, img = inputs(1, 2, 9, 33)
    before = ops.pairwise_affinity_loss(p, img, 5, 0.1, 0.0, True, 0).item()
    for window in (1, 4, 9):
        refused(lambda: ops.pairwise_affinity_loss(p, img, window, 0.1, 0.0, True, 0), "window must be 3, 5 or 7")
        if window > 1:           # (window 1 has no offsets: the empty output is refused as a null pointer)
            refused(lambda: ops.pairwise_cache(img, window, 0.1), "window must be 3, 5 or 7")
            refused(lambda: ops.compute_affinities(img, 0.1, 5, window), "window must be 3, 5 or 7")
    for window in (3, 5, 7):
        R = window // 2
        for H, W in ((R, 9), (9, R)):
            q, im = inputs(1, 2, H, W)
            refused(lambda: ops.pairwise_affinity_loss(q, im, window, 0.1, 0.0, True, 0), "reflect padding needs H, W > window/2")
            refused(lambda: ops.compute_affinities(im, 0.1, 5, window), "bad geometry")
    q, im = inputs(1, 33, 9, 33)
    refused(lambda: ops.pairwise_affinity_loss(q, im, 5, 0.1, 0.0, True, 0), "C <= 32")
    q, im = inputs(1, 28, 9, 33)
    refused(lambda: ops.pairwise_affinity_loss(q, im, 7, 0.1, 0.0, True, 0), "C too large for the LDS tile")
    refused(lambda: ops.pairwise_affinity_loss(p, img, 5, 0.0, 0.0, True, 0), "sigma_color must be positive")
    refused(lambda: ops.pairwise_cache(img, 5, 0.0), "sigma_color must be positive")
    refused(lambda: ops.compute_affinities(img, 0.0, 5, 5), "bad geometry")
    for other in (img[:, :, :8], img[:, :2], torch.cat([img, img])):
        refused(lambda: ops.pairwise_affinity_loss(p, other.contiguous(), 5, 0.1, 0.0, True, 0), "does not match preds", False)
    refused(lambda: ops.pairwise_affinity_loss(p.detach().cpu(), img, 5, 0.1, 0.0, True, 0), "needs a device tensor", False)
    refused(lambda: ops.pairwise_affinity_loss(p, img.cpu(), 5, 0.1, 0.0, True, 0), "needs a device tensor", False)
    refused(lambda: ops.pairwise_cache(img.cpu(), 5, 0.1), "needs a device tensor", False)
    refused(lambda: ops.compute_affinities(img.cpu(), 0.1, 5, 5), "needs a device tensor", False)
    refused(lambda: ops.pairwise_affinity_loss(p.double(), img, 5, 0.1, 0.0, True, 0), "expected torch.float32", False)
    assert ops.pairwise_affinity_loss(p, img, 5, 0.1, 0.0, True, 0).item() == before
