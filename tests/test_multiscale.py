"""Multi-scale + flip fusion without a device: the oracle of tests/multiscale_oracle.py against an independent formulation
(``F.interpolate`` in float64, ``torch.flip``, ``softmax`` / ``sigmoid``, a weighted mean / ``amax``), the float32 oracle's labels
within the cap the device test uses, ``multiscale_sizes``, every refusal that needs no device, and the callers' signatures."""
import inspect
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiscale_oracle as mo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def independent(case, act, red, weighted):
    (H, W), _sizes, mirrored, B, _C = mo.GEOMETRIES[case]
    srcs = mo.make_sources(case)
    w = mo.case_weights(case) if weighted else [1.0] * len(srcs)
    vals, ws = [], []
    for src, m, wk in zip(srcs, mirrored, w):
        r = F.interpolate(src.double(), size=(H, W), mode="bilinear", align_corners=False)
        for part in ([r[:B], torch.flip(r[B:], dims=(-1,))] if m else [r]):
            vals.append({"none": lambda t: t, "softmax": lambda t: torch.softmax(t, dim=1), "sigmoid": torch.sigmoid}[act](part))
            ws.append(wk)
    stack = torch.stack(vals)
    if red == "max":
        return stack.amax(dim=0)
    wt = torch.tensor(ws, dtype=torch.float64).view(-1, 1, 1, 1, 1)
    return (stack * wt).sum(dim=0) / wt.sum()


@pytest.mark.parametrize("case", range(len(mo.GEOMETRIES)))
def test_oracle_equals_the_independent_formulation(case):
    ref = mo.reference(case)
    assert len(ref["combos"]) in (6, 9)
    for (act, red, weighted), r in ref["combos"].items():
        want = independent(case, act, red, weighted)
        assert r["r64"].shape == want.shape
        err = (r["r64"] - want).abs().max().item()
        assert err <= 1e-12 * max(1.0, want.abs().max().item()), (case, act, red, weighted, err)
        # the float32 run stays a float32 run (its worst error: the rounded source coordinate times a step of the logits)
        assert r["yard"] <= 1e-3, (case, act, red, weighted, r["yard"])


def test_geometries_cover_what_the_kernels_branch_on():
    g = mo.GEOMETRIES
    assert len(g) == 24 and {t for t, *_ in g} == set(mo.TARGETS)
    assert {len(s) for _, s, *_ in g} == {1, 2, 4}
    assert {c for *_, c in g} == set(mo.CHANNELS) and {b for *_, b, _ in g} == {1, 3}
    kinds = set()
    for (H, W), sizes, mirrored, _b, _c in g:
        for (h, w), m in zip(sizes, mirrored):
            kinds.add(("one" if (h, w) == (1, 1) and (H, W) != (1, 1) else "equal" if (h, w) == (H, W) else
                       "larger" if h > H else "smaller", m))
    assert kinds == {(k, m) for k in ("one", "equal", "larger", "smaller") for m in (False, True)}


@pytest.mark.parametrize("case", range(len(mo.GEOMETRIES)))
def test_float32_oracle_labels_stay_within_the_exempt_cap(case):
    """Labels are compared where the float64 top-two margin exceeds twice the parity bound; that leaves out at most 0.1 % of
    the pixels, and the float32 oracle itself agrees with float64 on all the others (the combinations: ``mo.label_combos``)."""
    ref = mo.reference(case)["combos"]
    for act, red, weighted in mo.label_combos(mo.GEOMETRIES[case][4]):
        r = ref[(act, red, weighted)]
        b = mo.bound(r["r64"], r["yard"], mo.fused_coordinate_term(case, act)).amax(dim=1)
        sure = mo.label_margin(r["r64"]) > 2 * b
        assert (~sure).double().mean().item() <= 1e-3, (case, act, red, weighted)
        l64, _ = mo.labels(r["r64"])
        l32, _ = mo.labels(r["r32"])
        assert torch.equal(l64[sure], l32[sure]), (case, act, red, weighted)


def test_mirror_of_a_source_is_undone():
    """A source and its own mirror image fused with ``mirrored``: at the target's size exactly the source, elsewhere the
    fusion of the source alone up to the rounding of the mirrored coordinates."""
    g = torch.Generator().manual_seed(5)
    for (h, w), (H, W) in (((6, 9), (6, 9)), ((6, 9), (13, 20)), ((6, 8), (13, 21)), ((7, 5), (3, 4))):
        x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
        both = torch.cat([x, x.flip(-1)])
        got = mo.fuse([both], (H, W), mirrored=True)
        want = mo.fuse([x], (H, W))
        if (h, w) == (H, W):
            assert torch.equal(got, x)
        assert (got - want).abs().max().item() < 1e-12


def test_scale_flip_oracle_is_resize_then_mirror():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 9, 14, generator=g, dtype=torch.float64)
    for size in ((9, 14), (20, 31), (4, 5), (1, 1)):
        want = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        got = mo.scale_flip(x, size, True, torch.float64)
        assert (got[:2] - want).abs().max().item() < 1e-12 and torch.equal(got[2:], got[:2].flip(-1))
        assert torch.equal(mo.scale_flip(x, size, False, torch.float64), got[:2])
    assert torch.equal(mo.scale_flip(x, (9, 14), False, torch.float64), x)         # the input's own size: a copy


def test_labels_rule():
    s = torch.tensor([[[[0.2, 0.5, float("nan"), 0.1]], [[0.2, 0.4, 0.3, 0.3]], [[0.1, 0.5, 0.9, 0.05]]]])      # (1,3,1,4)
    lab, conf = mo.labels(s, min_conf=0.3, ignore_index=255)
    assert lab.tolist() == [[[255, 0, 0, 1]]]          # a tie takes the first; a NaN in channel 0 stays; below min_conf
    assert conf[0, 0, 1].item() == 0.5
    lab1, _ = mo.labels(torch.tensor([[[[0.5, 0.49, float("nan")]]]]), thresh=0.5)
    assert lab1.tolist() == [[[1, 0, 0]]]


def test_max_normalize_oracle():
    x = torch.tensor([[1.0, 4.0, -2.0], [0.0, 0.0, 0.0], [-1.0, -3.0, -2.0], [1.0, float("nan"), 2.0], [1.0, float("inf"), 2.0]])
    out, mask = mo.max_normalize(x, 0.25)
    assert out[0].tolist() == [0.25, 1.0, -0.5] and mask[0].tolist() == [1, 1, 0]
    for b in (1, 2, 3, 4):
        assert torch.equal(out[b].nan_to_num(7.0), x[b].nan_to_num(7.0))
    assert mask[1].tolist() == [0, 0, 0]            # v >= thresh && v > 0


def test_multiscale_sizes():
    from weaklysuperviseddl_amd import ops
    assert ops.multiscale_sizes(64, 64, (0.5, 1.0, 1.5)) == [(32, 32), (64, 64), (96, 96)]
    assert ops.multiscale_sizes(224, 224, (0.5, 1.0, 1.5, 2.0)) == [(128, 128), (224, 224), (352, 352), (448, 448)]   # 3.5 -> 4, 10.5 -> 11
    assert ops.multiscale_sizes(48, 80, (1.0,)) == [(64, 96)]                   # 1.5 -> 2 and 2.5 -> 3: halves go up
    assert ops.multiscale_sizes(48, 80, (1.0,), multiple=8) == [(48, 80)]
    assert ops.multiscale_sizes(100, 40, (0.1, 1.0), multiple=16) == [(16, 16), (96, 48)]     # never below one multiple
    assert ops.multiscale_sizes(512, 512, (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)) == [(256, 256), (384, 384), (512, 512), (640, 640),
                                                                              (768, 768), (896, 896)]
    for bad in ((0.0, 1.0), (-1.0,), (float("nan"),), (float("inf"),), (), tuple(1 + 0.5 * i for i in range(9)), "ab", (1.0, 1.01)):
        with pytest.raises(ValueError):
            ops.multiscale_sizes(64, 64, bad)
    with pytest.raises(ValueError):
        ops.multiscale_sizes(64, 64, (1.0,), multiple=0)
    with pytest.raises(ValueError):
        ops.multiscale_sizes(0, 64, (1.0,))


def test_refusals_need_no_device():
    from weaklysuperviseddl_amd import ops, WsdlError
    a = torch.zeros(2, 3, 4, 5)

    def refused(exc, match, *args, **kw):
        with pytest.raises(exc, match=match):
            ops.multiscale_fuse(*args, **kw)

    refused(WsdlError, "device tensor", [a], (8, 8))                                              # wrong device
    refused(WsdlError, "float32", [a.double()], (8, 8))                                           # wrong dtype
    refused(WsdlError, "holds 3 images", [a, torch.zeros(3, 3, 2, 2)], (8, 8))                    # batch mismatch
    refused(WsdlError, "channels", [a, torch.zeros(2, 4, 2, 2)], (8, 8))                          # channel mismatch
    refused(WsdlError, "odd", [torch.zeros(3, 3, 4, 5)], (8, 8), mirrored=True)                   # mirrored, odd leading dimension
    refused(WsdlError, "holds 1 images", [a, a], (8, 8), mirrored=[False, True])                  # halves do not match
    refused(WsdlError, "at most 64", [torch.zeros(1, 65, 2, 2)], (8, 8))                          # C > 64
    refused(ValueError, "1 to 8 sources", [a] * 9, (8, 8))
    refused(ValueError, "1 to 8 sources", [], (8, 8))
    refused(ValueError, "takes no weights", [a], (8, 8), reduce="max", weights=[1.0])
    refused(ValueError, "more than one channel", [torch.zeros(2, 1, 4, 5)], (8, 8), activation="softmax")
    refused(ValueError, "activation", [a], (8, 8), activation="relu")
    refused(ValueError, "reduce", [a], (8, 8), reduce="sum")
    refused(ValueError, "weights", [a, a], (8, 8), weights=[1.0])
    refused(ValueError, "weights", [a, a], (8, 8), weights=[0.0, 0.0])
    refused(ValueError, "weights", [a], (8, 8), weights=[-1.0])
    refused(ValueError, "mirrored flags", [a, a], (8, 8), mirrored=[True])
    refused(ValueError, "size", [a], (0, 8))
    refused(ValueError, "size", [a], 8)
    refused(WsdlError, "non-empty", [torch.zeros(2, 3, 4)], (8, 8))
    for call in (lambda: ops.scale_flip(a, (8, 8)), lambda: ops.max_normalize(a), lambda: ops.scale_flip(torch.zeros(3, 4, 5), (8, 8)),
                 lambda: ops.max_normalize(torch.zeros(4))):
        with pytest.raises(WsdlError):
            call()
    with pytest.raises(ValueError):
        ops.scale_flip(a, (8, 0))


def test_callers_keep_their_positional_signatures():
    from weaklysuperviseddl_amd.TraditionalModel import (evaluate_model, generate_pseudo_masks, predict_multiscale, LayerCAMGenerator,
                                                         SegmentationModel)
    from weaklysuperviseddl_amd.TraditionalModel import PsuedoMasks
    p = inspect.signature(evaluate_model).parameters
    assert list(p)[:4] == ["model", "loader", "device", "binarize"]
    assert p["device"].default == "cuda" and p["binarize"].default == "notebook"
    assert p["scales"].kind is p["flip"].kind is inspect.Parameter.KEYWORD_ONLY and p["scales"].default is None and p["flip"].default is False
    p = inspect.signature(generate_pseudo_masks).parameters
    assert list(p) == ["loader", "layercam_gen", "cam_thresh", "alpha", "keep_largest_masks", "run_id", "out_root", "max_images",
                       "write_png", "device", "rank", "world", "keep_images", "streams", "keep_on_device", "device_batch", "pamr",
                       "superpixels", "affinity", "boundary", "multiscale"]
    assert p["multiscale"].default is None and all(v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for v in p.values())
    p = inspect.signature(predict_multiscale).parameters
    assert p["scales"].default == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75) and p["flip"].default is True and p["activation"].default == "softmax"
    p = inspect.signature(LayerCAMGenerator.generate_multiscale).parameters
    assert list(p) == ["self", "images", "scales", "flip", "alpha", "class_idx", "thresh", "reduce", "multiple"]
    assert p["scales"].default == (0.5, 1.0, 1.5, 2.0)
    assert callable(SegmentationModel.head_logits)

    class Gen:                      # the refusals of multiscale= happen before the loader is touched
        generate_multiscale = None
    for kw in (dict(multiscale={"scale": 1}), dict(multiscale=[1.0]), dict(multiscale={}, device_batch=4)):
        with pytest.raises(ValueError, match="multiscale"):
            PsuedoMasks.generate_pseudo_masks(None, Gen(), write_png=False, **kw)
    with pytest.raises(ValueError, match="generate_multiscale"):
        PsuedoMasks.generate_pseudo_masks(None, object(), write_png=False, multiscale={})


def test_abi_table_and_build_list():
    from weaklysuperviseddl_amd import _lib, _build
    header = open(os.path.join(ROOT, "include", "wsdl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("wsdl_scale_flip", "wsdl_multiscale_fuse", "wsdl_plane_max_normalize", "wsdl_plane_max_workspace"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", code), name
    assert len(_lib.SIGNATURES["wsdl_multiscale_fuse"][1]) == 15 and len(_lib.SIGNATURES["wsdl_scale_flip"][1]) == 10
    assert "multiscale.hip" in _build.SOURCES and "multi-scale fusion" in header
    lib = _lib.lib()
    assert lib.wsdl_plane_max_workspace(0) == 0 and lib.wsdl_plane_max_workspace(65536) == 0 and lib.wsdl_plane_max_workspace(3) >= 12
    # host-side validation: refused without touching a device
    assert lib.wsdl_multiscale_fuse(None, 0, 1, 1, 1, 1, 0, 0, None, None, None, 0.5, 0.0, 255, None) != 0
    assert "sources" in lib.wsdl_last_error().decode()
    assert lib.wsdl_scale_flip(None, None, 1, 1, 1, 1, 1, 1, 0, None) != 0
