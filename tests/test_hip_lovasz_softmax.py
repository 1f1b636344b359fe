"""The multi-class Lovasz-softmax on the device at its edges: the segmented pipeline of csrc/lovasz_seg.hip - a class list
is one sort of all its entries, 'present' / 'all' sort class after class with a weight per image and class, one segment
sorts 32-bit keys and several 64-bit ones - against the tie-stable fp32 oracle
(tests/lovasz_softmax_oracle.py, pinned on the CPU by tests/test_lovasz_softmax.py).  The oracle orders equal errors by pixel
index, as the kernels document, so every case compares the loss and the WHOLE gradient - no pixel is masked out, the
pixels inside a tie least of all.  Tolerances are the project's: loss 1e-5 of max(1, |loss|); gradient 1e-5 max|grad| + 1e-9,
and 2e-4 max|grad| in the one case of more than a million pixels in a segment.  Every case runs twice and must repeat bit for bit.
Where both run, classes='all' and classes=list(range(C)) - C sorts and one, the same kernels - must give the same gradient
bit for bit and losses within 1e-6 (the number of partial sums differs).
The worst measured errors of each group are reported with ``report_line``."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_softmax_oracle as S  # noqa: E402
from conftest import report_line  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def worst():
    """group -> [loss error / its bound's scale, gradient error / max|grad|, cases]; 'cross' -> the same for 'all' against the list."""
    w = {}
    yield w
    for group, (e_loss, e_grad, n, tol) in w.items():
        if group == "cross":
            continue
        report_line(f"lovasz_softmax {group}: {n} runs, worst |device - oracle|: loss {e_loss:.2e} of max(1, |loss|) (held to 1e-5), "
                    f"gradient {e_grad:.2e} of max|grad| (held to {tol})")
    if "cross" in w:
        e_loss, e_grad, n, same = w["cross"]
        report_line(f"lovasz_softmax 'all' against list(range(C)): {n} cases, worst relative difference: loss {e_loss:.2e} (held to "
                    f"1e-6), gradient {e_grad:.2e} of max|grad| (held to bit-identity); bit-identical loss too in {same} of them")


def on_device(dev, p, lab, classes, per_image, ignore):
    from weaklysuperviseddl_amd import ops
    pd = p.to(dev).requires_grad_()
    loss = ops.lovasz_softmax(pd, lab.to(dev), classes, per_image, ignore)
    loss.backward()
    return loss.item(), pd.grad.cpu()


def run_case(dev, worst, group, name, p, lab, modes, per_image=False, ignore=None, big=False):
    """modes: 'present', 'all', 'list' (= list(range(C))) or an explicit list.  Returns mode -> (loss, gradient) of the device."""
    C = 1 if p.dim() == 3 else p.shape[1]
    out, ref = {}, {}
    for mode in modes:
        classes = list(range(C)) if mode == "list" else mode
        key = "all" if mode == "list" else str(mode)                     # the list of all classes is 'all': one reference
        if key not in ref:
            ref[key] = S.loss_and_grad(p, lab, classes, per_image, ignore)
        want_loss, want = ref[key]
        loss, grad = on_device(dev, p, lab, classes, per_image, ignore)
        scale = want.abs().max().item()
        e_loss = abs(loss - want_loss) / max(1.0, abs(want_loss))
        e_grad = (grad - want).abs().max().item()
        print(f"{group} / {name} / {mode}: loss {loss:.9g} oracle {want_loss:.9g} (|d| / scale {e_loss:.3e}); gradient max|d| "
              f"{e_grad:.3e} of max|oracle| {scale:.3e}")
        tol = "2e-4" if big else "1e-5 + 1e-9"
        assert loss == loss and bool(torch.isfinite(grad).all()), (group, name, mode, "loss", loss, "oracle", want_loss)
        assert e_loss <= 1e-5, (group, name, mode, loss, want_loss)
        assert e_grad <= (2e-4 * scale if big else 1e-5 * scale + 1e-9), (group, name, mode, e_grad, scale)
        assert (1 if per_image else p.shape[0]) * p.shape[-2] * p.shape[-1] < 1000000 or big     # the pixels of one sort's segment
        w = worst.setdefault(group, [0.0, 0.0, 0, tol])
        w[0], w[1], w[2] = max(w[0], e_loss), max(w[1], e_grad / scale if scale > 0 else e_grad), w[2] + 1
        loss2, grad2 = on_device(dev, p, lab, classes, per_image, ignore)
        assert loss2 == loss and torch.equal(grad2, grad), (group, name, mode, "two runs differ")
        out[str(mode)] = (loss, grad)
    if "all" in out and "list" in out:
        (la, ga), (ll, gl) = out["all"], out["list"]
        scale = ga.abs().max().item()
        d_loss = abs(la - ll) / max(abs(la), abs(ll)) if la != ll else 0.0
        d_grad = (ga - gl).abs().max().item() / scale if scale > 0 else (ga - gl).abs().max().item()
        same = la == ll and torch.equal(ga, gl)
        print(f"{group} / {name}: 'all' against the list: loss {la:.9g} / {ll:.9g} (relative {d_loss:.3e}), gradient {d_grad:.3e} of "
              f"max|grad|; bit-identical: {same}")
        assert d_loss <= 1e-6 and torch.equal(ga, gl), (group, name, la, ll, d_grad)
        w = worst.setdefault("cross", [0.0, 0.0, 0, 0])
        w[0], w[1], w[2], w[3] = max(w[0], d_loss), max(w[1], d_grad), w[2] + 1, w[3] + int(same)
    return out


THREE = ("list", "present", "all")


# ------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("kind", ["eighths", "one-hot"])
@pytest.mark.parametrize("shape", [(2, 3, 9, 13), (1, 2, 1, 300)])
def test_ties_are_ordered_by_pixel_index(dev, worst, shape, kind):
    """Probabilities in multiples of 1/8 (renormalised: exact 0 and 1 occur) and one-hot ones tie whole groups of pixels; the
    gradient depends on the rank inside each group."""
    gen = torch.Generator().manual_seed(31)
    B, C, H, W = shape
    p = S.quantised_probas(shape, gen) if kind == "eighths" else S.one_hot_probas(shape, gen)
    lab = torch.randint(0, C, (B, H, W), generator=gen)
    assert (p == 0).any() and (p == 1).any()
    e = (torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).float() - p).abs()
    assert all(torch.unique(e[:, c]).numel() < e[:, c].numel() // 4 for c in range(C))       # ties in every class
    out = run_case(dev, worst, "ties", f"{kind} {shape}", p, lab, THREE)
    assert out["all"][1].abs().max().item() > 0


# ---------------------------------------------------------------------------------- void pixels that tie with valid ones
def void_zero_input(where):
    """1 x 3 x 4 x 5: class 2 absent and its probability exactly 0 at every pixel, so all its errors are 0.  An ignored pixel
    keyed like an error of 0 would, at a lower index, sort in front of valid ones: it has to sort strictly behind them."""
    gen = torch.Generator().manual_seed(32)
    p = torch.zeros(1, 3, 4, 5)
    p[:, :2] = torch.softmax(torch.randn(1, 2, 4, 5, generator=gen), 1)
    lab = torch.randint(0, 2, (1, 4, 5), generator=gen)
    lab.view(-1)[{"first": [0], "last": [19], "scattered": [0, 1, 6, 12, 19]}[where]] = 255
    assert (p[:, 2] == 0).all() and not (lab == 2).any() and (lab == 0).any() and (lab == 1).any()
    return p, lab


@pytest.mark.parametrize("mode", THREE)
@pytest.mark.parametrize("where", ["first", "last", "scattered"])
def test_void_pixels_among_zero_errors(dev, worst, where, mode):
    """Finite, and the oracle's: the reference removes void pixels before it sorts, the absent class is a zero term ('all') or
    none ('present').  Before ignored pixels were keyed strictly below every valid pixel, 'present' and 'all' gave NaN with
    pixel 0 void: J of an empty prefix with G = 0 is 1 - 0 / 0."""
    p, lab = void_zero_input(where)
    out = run_case(dev, worst, "void and zero error", f"void {where}", p, lab, [mode], ignore=255)
    loss, grad = out[mode]
    assert (grad[:, :, lab[0] == 255] == 0).all() and (grad[:, 2] == 0).all() and loss > 0


@pytest.mark.parametrize("per_image", [False, True])
def test_all_void_batch_is_zero(dev, per_image):
    from weaklysuperviseddl_amd import ops
    gen = torch.Generator().manual_seed(33)
    p = torch.softmax(torch.randn(2, 3, 4, 5, generator=gen), 1)
    lab = torch.full((2, 4, 5), 255)
    for classes in ("present", "all", [0, 2]):
        assert S.lovasz_softmax(p, lab, classes, per_image, 255).item() == 0.0
        runs = [on_device(dev, p, lab, classes, per_image, 255) for _ in range(2)]
        for loss, grad in runs:
            assert loss == 0.0 and (grad == 0).all(), (classes, per_image, loss)
    assert ops.lovasz_softmax(p.to(dev), lab.to(dev), "all", per_image, 255).item() == 0.0          # and without a gradient


# ----------------------------------------------------------------------------------------------------------- class counts
def labels_with_absent_classes(C, shape, gen):
    """C <= 2: labels 1 and 2 (2 is no class there: valid background of every class), class 0 absent; else classes 0, 3 and
    C - 1 absent."""
    if C <= 2:
        return torch.randint(1, 3, shape, generator=gen)
    lab = torch.randint(0, C, shape, generator=gen)
    lab[(lab == 0) | (lab == 3) | (lab == C - 1)] = 1
    return lab


@pytest.mark.parametrize("C", [1, 2, 8, 9, 21])
def test_class_counts(dev, worst, C):
    """C <= 8: per-thread counters of the histogram; beyond: its LDS path.  Some classes are absent, so 'present' and 'all'
    average over different sets."""
    gen = torch.Generator().manual_seed(34 + C)
    shape = (2, C, 7, 11)
    p = torch.rand(shape, generator=gen) if C == 1 else torch.softmax(torch.randn(shape, generator=gen), 1)
    lab = labels_with_absent_classes(C, (2, 7, 11), gen)
    out = run_case(dev, worst, "class counts", f"C={C}", p, lab, THREE)
    assert out["present"][0] != out["all"][0] and not torch.equal(out["present"][1], out["all"][1])
    if C == 1:                                                              # one sigmoid map (B,H,W) and one listed class
        run_case(dev, worst, "class counts", "C=1 map", p[:, 0].contiguous(), lab, [[1]])


def test_class_count_beyond_the_lds_histogram(dev, worst):
    """C = 1030: labels below 1024 are counted in LDS, the others straight in memory.  (A class list holds at most 1024
    entries, so the list of all classes does not exist here; a short list runs instead.)"""
    gen = torch.Generator().manual_seed(35)
    C = 1030
    p = torch.softmax(torch.randn(1, C, 2, 5, generator=gen), 1)
    lab = torch.tensor([0, 5, 1023, 1024, 1029, 1029, 7, 1025, 5, 600]).view(1, 2, 5)
    out = run_case(dev, worst, "class counts", "C=1030", p, lab, ["present", "all", [1029, 1024, 5, 1023, 2]])
    assert out["present"][0] != out["all"][0] and not torch.equal(out["present"][1], out["all"][1])
    present = sorted(set(lab.view(-1).tolist()))
    assert (out["present"][1][0, [c for c in range(C) if c not in present]] == 0).all()
    assert all(out["present"][1][0, c].abs().max().item() > 0 for c in present)


# ---------------------------------------------------------------------------------------- labels that are no class, not void
@pytest.mark.parametrize("ignore", [None, 254])
def test_labels_out_of_range_are_background(dev, worst, ignore):
    """-3, C and 255 are in no class and are not the ignore label: valid background for every class."""
    gen = torch.Generator().manual_seed(36)
    p = torch.softmax(torch.randn(2, 3, 5, 7, generator=gen), 1)
    lab = torch.randint(0, 3, (2, 5, 7), generator=gen)
    r = torch.rand(2, 5, 7, generator=gen)
    odd = (255,) if ignore is not None else (-3, 3, 255)
    for j, v in enumerate(odd):
        lab[(r >= 0.1 * j) & (r < 0.1 * (j + 1))] = v
    if ignore is not None:
        lab[r > 0.85] = ignore
    outside = (lab < 0) | ((lab >= 3) & (lab != (ignore if ignore is not None else -1)))
    assert all((lab == v).any() for v in odd) and (ignore is None or (lab == ignore).any())
    out = run_case(dev, worst, "labels out of range", f"ignore={ignore}", p, lab, THREE, ignore=ignore)
    for mode in THREE:
        g = out[mode][1].permute(1, 0, 2, 3)[:, outside]
        assert (g > 0).any() and not (g < 0).any(), mode                   # background: the loss grows with p
        if ignore is not None:
            assert (out[mode][1].permute(1, 0, 2, 3)[:, lab == ignore] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- grid edges
@pytest.mark.parametrize("P", [1, 255, 257, 1024 * 256 + 3])
def test_whole_batch_grid_edges(dev, worst, P):
    """One pixel, one short of / one past a workgroup, and three past 1024 x 256: the apply kernel's parts (at most
    1024 sorted positions each, 257 of them in the last case) are ragged and the key kernel's last workgroup is partly idle."""
    gen = torch.Generator().manual_seed(37)
    p = torch.softmax(torch.randn(1, 2, 1, P, generator=gen), 1)
    lab = torch.randint(0, 2, (1, 1, P), generator=gen) if P > 1 else torch.ones(1, 1, 1, dtype=torch.long)
    run_case(dev, worst, "grid edges, whole batch", f"P={P}", p, lab, THREE)


def test_whole_batch_beyond_the_grid(dev, worst):
    """1 x 3 x 1031 x 1021 > 4096 x 256 pixels: the grid-stride loops of the key and histogram kernels take one more
    trip for some threads only.  Scattered void, class 2 absent.  The one case of more than a million pixels."""
    gen = torch.Generator().manual_seed(38)
    shape = (1, 3, 1031, 1021)
    assert shape[2] * shape[3] > 4096 * 256
    p = torch.softmax(torch.randn(shape, generator=gen), 1)
    lab = torch.randint(0, 2, (1, 1031, 1021), generator=gen)
    lab[torch.rand(1, 1031, 1021, generator=gen) < 0.05] = 255
    out = run_case(dev, worst, "beyond a million pixels", str(shape), p, lab, THREE, ignore=255, big=True)
    assert out["present"][0] != out["all"][0]
    assert (out["all"][1].permute(1, 0, 2, 3)[:, lab == 255] == 0).all()


def max_parts():
    src = open(os.path.join(ROOT, "weaklysuperviseddl_amd", "csrc", "lovasz_seg.hip")).read()
    return int(re.search(r"constexpr int kMaxParts = (\d+);", src).group(1))


def test_class_list_more_segments_than_parts(dev, worst):
    """per_image with B K just past kMaxParts: kMaxParts / S == 0 and every segment is one part."""
    K = 3
    B = max_parts() // K + 1
    assert B * K > max_parts() >= (B - 1) * K
    gen = torch.Generator().manual_seed(39)
    p = torch.softmax(torch.randn(B, K, 3, 5, generator=gen), 1)
    lab = torch.randint(0, K, (B, 3, 5), generator=gen)
    lab[torch.rand(B, 3, 5, generator=gen) < 0.1] = 255
    lab[5] = 255
    run_case(dev, worst, "grid edges, class list", f"S={B * K}", p, lab, ["list"], per_image=True, ignore=255)


def test_class_list_ragged_last_part(dev, worst):
    """L = 1025, one segment: two parts (513 and 512 sorted positions), the second starts inside the segment."""
    gen = torch.Generator().manual_seed(40)
    p = torch.softmax(torch.randn(1, 2, 1, 1025, generator=gen), 1)
    lab = torch.randint(0, 2, (1, 1, 1025), generator=gen)
    run_case(dev, worst, "grid edges, class list", "L=1025", p, lab, [[1]])


@pytest.mark.parametrize("per_image", [False, True])
def test_class_listed_twice(dev, worst, per_image):
    """[1, 1, 0]: the two entries of class 1 add their equal terms to one plane with atomicAdd.  Against [1, 2, 0] - the same
    three segments' weight, class 1 listed once - plane 1 is twice the single entry's gradient to 1 ulp, plane 0 the same."""
    gen = torch.Generator().manual_seed(41)
    p = torch.softmax(torch.randn(2, 3, 5, 7, generator=gen), 1)
    lab = torch.randint(0, 3, (2, 5, 7), generator=gen)
    out = run_case(dev, worst, "grid edges, class list", f"[1, 1, 0] per_image={per_image}", p, lab, [[1, 1, 0]], per_image=per_image)
    _loss, twice = out[str([1, 1, 0])]
    _l1, once = on_device(dev, p, lab, [1, 2, 0], per_image, None)
    assert once[:, 1].abs().max().item() > 0
    ulp = torch.nextafter(2 * once[:, 1].abs(), torch.full_like(once[:, 1], float("inf"))) - 2 * once[:, 1].abs()
    assert ((twice[:, 1] - 2 * once[:, 1]).abs() <= ulp).all()
    assert torch.equal(twice[:, 0], once[:, 0]) and (twice[:, 2] == 0).all()


# ------------------------------------------------------------------------------------------------------ per image with ignore
def test_per_image_with_ignore(dev, worst):
    """3 x 3 x 6 x 7: image 0 entirely void (a zero term that counts), image 1 without class 2, image 2 with scattered void."""
    gen = torch.Generator().manual_seed(42)
    p = torch.softmax(torch.randn(3, 3, 6, 7, generator=gen), 1)
    lab = torch.randint(0, 3, (3, 6, 7), generator=gen)
    lab[0] = 255
    lab[1][lab[1] == 2] = 0
    lab[2][torch.rand(6, 7, generator=gen) < 0.2] = 255
    assert (lab[2] == 2).any() and (lab[2] == 255).any()
    out = run_case(dev, worst, "per image with ignore", "3x3x6x7", p, lab, THREE, per_image=True, ignore=255)
    assert (out["present"][1][0] == 0).all() and (out["present"][1][1, 2] == 0).all() and out["present"][1][2, 2].abs().max() > 0
    assert out["present"][0] != out["all"][0]


# ------------------------------------------------------------------------------- per image: the images are segments of one sort
def per_image_ragged_input():
    """3 x 3 x 1 x 1025: two parts per segment, the second ragged (513 and 512 sorted positions).  Image 1 lacks class 2,
    image 2 has scattered void: the images average over 3, 2 and 3 classes, so their weights differ."""
    gen = torch.Generator().manual_seed(43)
    p = torch.softmax(torch.randn(3, 3, 1, 1025, generator=gen), 1)
    lab = torch.randint(0, 3, (3, 1, 1025), generator=gen)
    lab[1][lab[1] == 2] = 0
    lab[2][torch.rand(1, 1025, generator=gen) < 0.2] = 255
    assert all((lab[b] == c).any() for b in (0, 2) for c in range(3)) and (lab[2] == 255).any()
    return p, lab


def per_image_capped_parts_input():
    """B x 2 x 1 x L with B = kMaxParts / 32 images and L three past 1024 x 32: every segment wants 33 parts and is granted
    kMaxParts / B = 32.  Image 0 lacks class 1."""
    B = max_parts() // 32
    L = 1024 * 32 + 3
    assert (L + 1023) // 1024 == 33 and max_parts() // B == 32
    gen = torch.Generator().manual_seed(44)
    p = torch.softmax(torch.randn(B, 2, 1, L, generator=gen), 1)
    lab = torch.randint(0, 2, (B, 1, L), generator=gen)
    lab[0] = 0
    return p, lab


def per_image_one_part_each_input():
    """B x 3 x 3 x 5 with B one past kMaxParts: kMaxParts / S == 0 and every segment is one part.  Image 5 is void, image 7
    lacks class 2, void pixels are scattered over the others."""
    B = max_parts() + 1
    gen = torch.Generator().manual_seed(45)
    p = torch.softmax(torch.randn(B, 3, 3, 5, generator=gen), 1)
    lab = torch.randint(0, 3, (B, 3, 5), generator=gen)
    lab[torch.rand(B, 3, 5, generator=gen) < 0.1] = 255
    lab[5] = 255
    lab[7][lab[7] == 2] = 0
    return p, lab


@pytest.mark.parametrize("make", [per_image_ragged_input, per_image_capped_parts_input, per_image_one_part_each_input])
def test_per_image_segments(dev, worst, make):
    """'present' / 'all' per image: the count at a segment's start is subtracted for every image but the first, and every
    (image, class) has a weight of its own - 1 / (classes of the image x images), 0 for a class the image lacks."""
    p, lab = make()
    out = run_case(dev, worst, "per image segments", make.__name__, p, lab, THREE, per_image=True, ignore=255)
    assert out["present"][0] != out["all"][0] and not torch.equal(out["present"][1], out["all"][1])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(dev):
    from weaklysuperviseddl_amd import WsdlError, _lib, ops
    lib = _lib.lib()
    p = torch.softmax(torch.randn(1, 2, 4, 5), 1).to(dev)
    lab = torch.zeros(1, 4, 5, dtype=torch.long, device=dev)
    loss = torch.full((), 123.0, device=dev)
    dp = torch.full_like(p, 7.0)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    cls = (ctypes.c_int * 1)(1)
    cp = ctypes.cast(cls, ctypes.c_void_p)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = [t.data_ptr() for t in (p, lab, loss, dp)]
    # 2^30 pixels: the small buffers are never touched
    assert lib.wsdl_lovasz_softmax_fwd_bwd(*ptr, 1, 2, 32768, 32768, 0, 0, -1, ws.data_ptr(), ws.numel(), stream) == -1
    assert b"2^30" in lib.wsdl_last_error()
    assert lib.wsdl_lovasz_softmax_classes_fwd_bwd(*ptr, 1, 2, 32768, 32768, cp, 1, 0, -1, ws.data_ptr(), ws.numel(), stream) == -1
    assert b"2^30" in lib.wsdl_last_error()
    # a workspace one byte short: WSDL_EWORKSPACE (-3)
    for per_image in (0, 1):
        need = lib.wsdl_lovasz_softmax_workspace(1, 2, 4, 5, per_image)
        assert 0 < need <= ws.numel()
        assert lib.wsdl_lovasz_softmax_fwd_bwd(*ptr, 1, 2, 4, 5, 0, per_image, -1, ws.data_ptr(), need - 1, stream) == -3
        assert b"workspace" in lib.wsdl_last_error()
    need = lib.wsdl_lovasz_softmax_classes_workspace(1, 2, 4, 5, 1, 0)
    assert 0 < need <= ws.numel()
    assert lib.wsdl_lovasz_softmax_classes_fwd_bwd(*ptr, 1, 2, 4, 5, cp, 1, 0, -1, ws.data_ptr(), need - 1, stream) == -3
    assert b"workspace" in lib.wsdl_last_error()
    torch.cuda.synchronize()
    assert loss.item() == 123.0 and (dp == 7.0).all()                      # nothing was launched, not even the memsets
    assert lib.wsdl_lovasz_softmax_fwd_bwd(*ptr, 1, 2, 4, 5, 0, 0, -1, ws.data_ptr(), ws.numel(), stream) == 0  # the buffers are fine
    torch.cuda.synchronize()
    assert loss.item() != 123.0 and not (dp == 7.0).any()
    for classes in ("present", "all", [1]):
        with pytest.raises(WsdlError, match="int64"):
            ops.lovasz_softmax(p, lab.float(), classes)                    # float labels
        with pytest.raises(WsdlError, match="int64"):
            ops.lovasz_softmax(p, lab.int(), classes)
        with pytest.raises(WsdlError, match="no CPU fallback"):
            ops.lovasz_softmax(p.cpu(), lab.cpu(), classes)
        with pytest.raises(WsdlError, match="no CPU fallback"):
            ops.lovasz_softmax(p, lab.cpu(), classes)
    with pytest.raises(WsdlError, match="empty class list"):
        ops.lovasz_softmax(p, lab, [])
    with pytest.raises(WsdlError):
        ops.lovasz_softmax(p, lab, list(range(2)) * 513)                   # 1026 entries: more than a list holds
    with pytest.raises(WsdlError):
        ops.lovasz_softmax(p, lab, "some")
