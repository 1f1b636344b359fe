"""The cases behind tests/golden/softmax_loss_bits.npz: seeded numpy inputs and the device calls whose results are recorded
as bit patterns - shared by tests/golden/make_softmax_loss_bits.py (which writes the file) and
tests/test_hip_softmax_loss_bits.py (which compares with it).  The four float64 softmax kernels (boundary loss, overlap sums,
Tversky gradient, focal loss) promise bitwise reproducible results; the file pins the bits, so a change of their shared
frame that alters one rounding or the order of one sum is seen.

Small cases (B = 2, the whole gradient stored): C = 2, 3, 5 (registers for 2 and 3, the re-reading form for 5) on
  vector   6 x 10: H W a multiple of 4, every pointer aligned - items of four pixels
  scalar   5 x 7:  H W odd - items of one pixel
  offset   6 x 10 logits at a storage offset of one float: the vector shape, which must take the scalar path
Large cases (B = 1; the loss, the sum of the gradient's words and its first and last 64 words stored): every grid-stride
loop wraps and the partials fill their cap."""
import numpy as np
import torch

IGNORE = 255
LAYOUTS = {"vector": (6, 10), "scalar": (5, 7), "offset": (6, 10)}
SMALL = [(C, layout) for C in (2, 3, 5) for layout in LAYOUTS]
LARGE = {
    "vector_1028x1024": (1, 2, 1028, 1024),      # 1 052 672 pixels: wraps the 1024-workgroup fused passes and the 2048-workgroup sums
    "scalar_1025x1025": (1, 3, 1025, 1025),      # 1 050 625 pixels, H W odd: wraps every scalar loop, the 4096-workgroup gradient too
    "tversky_2052x2048": (1, 2, 2052, 2048),     # wraps the vector gradient loop (Tversky only)
}
TVERSKY = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0)


def class_lists(C):
    return [cl for cl in ((1,), (2, 0), tuple(range(C))) if max(cl) < C]


def make_inputs(B, C, H, W, seed):
    """float32 logits (normal x 4), int64 labels with about 10 % ignored, float32 phi (B,C,H,W), pixel and class weights."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C, H, W)) * 4).astype(np.float32)
    labels = rng.integers(0, C, (B, H, W)).astype(np.int64)
    labels[rng.random((B, H, W)) < 0.1] = IGNORE
    phi = (rng.standard_normal((B, C, H, W)) * 3).astype(np.float32)
    pixel_weight = rng.random((B, H, W)).astype(np.float32)
    pixel_weight[rng.random((B, H, W)) < 0.05] = 0.0
    class_weight = (0.5 + rng.random(C)).astype(np.float32)
    return logits, labels, phi, pixel_weight, class_weight


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def on_device(logits, dev, offset):
    """The logits as a leaf on the device; with ``offset`` a contiguous view one float into its storage (4-byte aligned only)."""
    src = torch.from_numpy(logits)
    if not offset:
        return src.to(dev).requires_grad_()
    store = torch.empty(src.numel() + 1, device=dev, dtype=torch.float32)
    z = store[1:].view(src.shape)
    z.copy_(src)
    assert z.data_ptr() % 16 == 4 and z.is_contiguous()
    return z.detach().requires_grad_()


def calls(C, inputs, dev, small):
    """[(name, fn(z) -> tensor)] - every recorded call on logits ``z``; ``small`` adds the variants the large cases leave out."""
    from weaklysuperviseddl_amd import ops
    _, labels, phi, pixel_weight, class_weight = inputs
    y = torch.from_numpy(labels).to(dev)
    ph, pw, cw = (torch.from_numpy(a).to(dev) for a in (phi, pixel_weight, class_weight))
    scale = torch.tensor([1.5], device=dev)
    out = []
    for cl in class_lists(C) if small else [tuple(range(C))]:
        tag = "".join(str(c) for c in cl)
        p = ph[:, list(cl)].contiguous()
        out.append((f"boundary/{tag}", lambda z, cl=cl, p=p: ops.boundary_loss(z, p, y, classes=cl, ignore_index=IGNORE,
                                                                               scale=scale if len(cl) == 1 else None)))
        out.append((f"sums/{tag}", lambda z, cl=cl: ops.overlap_sums(z, y, classes=cl, ignore_index=IGNORE)))
        out.append((f"tversky/{tag}", lambda z, cl=cl: ops.tversky_loss(z, y, classes=cl, ignore_index=IGNORE, **TVERSKY)))
        if small:
            out.append((f"boundary_nolabels/{tag}", lambda z, cl=cl, p=p: ops.boundary_loss(z, p, None, classes=cl)))
            out.append((f"sums_per_image/{tag}", lambda z, cl=cl: ops.overlap_sums(z, y, classes=cl, ignore_index=IGNORE, per_image=True)))
            out.append((f"tversky_per_image/{tag}", lambda z, cl=cl: ops.tversky_loss(z, y, classes=cl, ignore_index=IGNORE, per_image=True,
                                                                                      scale=scale if len(cl) == 1 else None, **TVERSKY)))
    out.append(("focal_mean", lambda z: ops.focal_loss(z, y, gamma=2.0, ignore_index=IGNORE)))
    if small:
        out.append(("tversky_present_only", lambda z: ops.tversky_loss(z, y, ignore_index=IGNORE, per_image=True, present_only=True)))
        out.append(("focal_none", lambda z: ops.focal_loss(z, y, gamma=2.0, ignore_index=IGNORE, reduction="none")))
        out.append(("focal_weighted", lambda z: ops.focal_loss(z, y, gamma=1.5, weight=cw, pixel_weight=pw, ignore_index=IGNORE)))
    return out


def run(fn, z):
    """-> (result, gradient or None): the call, and ``.backward()`` where the result has a gradient."""
    z.grad = None
    res = fn(z)
    if not res.requires_grad:
        return res, None
    (res.sum() if res.dim() else res).backward()
    return res, z.grad


def record_small(dev, C, layout):
    H, W = LAYOUTS[layout]
    inputs = make_inputs(2, C, H, W, 1000 * C + list(LAYOUTS).index(layout))
    z = on_device(inputs[0], dev, layout == "offset")
    out = {}
    for name, fn in calls(C, inputs, dev, True):
        res, grad = run(fn, z)
        out[f"C{C}_{layout}/{name}/value"] = bits(res)
        if grad is not None:
            out[f"C{C}_{layout}/{name}/grad"] = bits(grad)
    return out


def record_large(dev, case):
    B, C, H, W = LARGE[case]
    inputs = make_inputs(B, C, H, W, 7000 + list(LARGE).index(case))
    z = on_device(inputs[0], dev, False)
    out = {}
    for name, fn in calls(C, inputs, dev, False):
        if case.startswith("tversky") and not name.startswith("tversky"):
            continue
        res, grad = run(fn, z)
        out[f"{case}/{name}/value"] = bits(res)
        if grad is not None:
            w = bits(grad).ravel()
            out[f"{case}/{name}/grad_sum"] = np.array(w.sum(dtype=np.uint64))
            out[f"{case}/{name}/grad_head"] = w[:64].copy()
            out[f"{case}/{name}/grad_tail"] = w[-64:].copy()
    return out
