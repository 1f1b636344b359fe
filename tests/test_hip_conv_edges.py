"""The implicit-GEMM convolutions at the edges the full-size test (tests/test_hip_conv_fullsize.py) does not reach: ragged
shapes in every tile configuration, the fused epilogue and its published amax, strided operands and accumulate forms, and
geometry outside 'same' padding - all against float64 on the host (tests/conv_oracle.py), per channel, at 1e-4.

1. RAGGED: the smallest shapes whose launch trace shows each configuration of ``launch_igemm`` (chosen with the trace, from the
   dispatch rules): B*OH*OW and OH*OW are no multiples of the pixel tile (an image boundary falls inside a tile), H != W,
   Cout is no multiple of the row tile and Cin is the smallest the configuration admits - wherever its eligibility rule allows
   (``split<64,64,32>`` needs Cout % 64 == 0, a non-zero ``xcd_py`` a tile count that is a multiple of 8, ``ks=2`` 64 K chunks of
   32: Cin = 256).  A forward shape (Cin, Cout) has a twin (Cout, Cin) whose INPUT GRADIENT runs the same configuration.
2. The epilogue ``relu(scale * conv + shift + residual)`` in seven term sets on every forward shape of 1, and max|y| as the
   kernels publish it: equal to ``out.abs().max()`` bit for bit from the split epilogue, both split-K reduce kernels, the stem
   and the read pass behind the fp32 kernels.
3. x / out / residual / dy as channel slices of wider tensors (batch strides that are and are not multiples of 4 floats),
   ``conv2d_dgrad(accumulate_into=, acc_mask=)`` in every input-gradient configuration of 1, ``conv2d_fwd_group`` and
   ``conv2d_dgrad_multi`` on non-square maps with more than one column band.
4. Padding 0 and beyond 'same', stride 2 with dilation 2, pad < dilation, 5x5, 1x1 stride 3, dilation 12 on a map narrower than
   12 in one dimension: the library either matches float64 in all three passes or raises ``WsdlError`` without a launch.
   Refusals: none - every geometry of ``GEOMETRIES`` is computed (the 5x5 ones on the fp32 kernels: 25 taps are not
   split-eligible).

Time on an MI355X box (16 host threads for the float64 references): the whole file 5.4 s for 124 cases; the slowest case 0.6 s
(``test_ragged_shape_vs_float64[t256]``, which also pays the library's first launches), every other one below 0.35 s; the float64
references of all 34 ragged shapes together 2 s (the heaviest, ``t256 ks=2``: 17.7 GFLOP, 0.15 s with its five device runs).
"""
import contextlib
import time
import zlib

import numpy as np
import pytest
import torch

from conftest import cpu_threads, report_line
from conv_oracle import ARITHMETICS, DEFAULTS, PASS_NAME, TOL, Table, chan_err, config_key, dgrad64, fwd64, pass_err, set_options, wgrad64

pytestmark = pytest.mark.gpu

PLAIN = "fp16x2 plain loop"

# (name, (B, Cin, H, W, Cout, k, stride, pad, dil), passes compared)
RAGGED = [
    # 256 x 128 tiles: >= 256 workgroups of them, >= 400 tiles of 128 x 128, rows >= 90 % of the row tiles
    ("t256", (3, 16, 75, 73, 504, 3, 1, 1, 1), "f"),                    # 129 x 2 workgroups; il=1, and il=0 under conv_il=0
    ("t256 twin", (3, 504, 75, 73, 16, 3, 1, 1, 1), "d"),
    ("t256 ks=2", (6, 256, 53, 52, 232, 3, 1, 1, 1), "f"),              # 260 tiles of 128 x 128, 72 chunks of 32: two K slices
    ("t256 ks=2 twin", (6, 232, 53, 52, 256, 3, 1, 1, 1), "d"),
    ("t256 xcd", (3, 16, 50, 54, 1000, 3, 1, 1, 1), "f"),               # 64 x 4 workgroups, weights the larger operand: xcd_py=4
    ("t256 xcd twin", (3, 1000, 50, 54, 16, 3, 1, 1, 1), "d"),
    ("t256 bands", (3, 16, 133, 41, 504, 3, 1, 12, 12), "f"),           # column bands [0,12) [12,29) [29,41)
    ("t256 bands twin", (3, 504, 133, 41, 16, 3, 1, 12, 12), "d"),
    ("128x128", (3, 16, 92, 93, 200, 3, 1, 1, 1), "f"),                 # 201 x 2 tiles, rows 78 % of a 256-row tile
    ("128x128 twin", (3, 200, 92, 93, 16, 3, 1, 1, 1), "d"),
    ("128x64 bk16", (2, 16, 19, 23, 104, 3, 1, 1, 1), "f"),
    ("128x64 bk16 twin", (2, 104, 19, 23, 16, 3, 1, 1, 1), "d"),
    ("128x64 bk32", (3, 32, 59, 58, 104, 3, 1, 1, 1), "f"),             # 161 tiles of 128 x 64: no split-K
    ("128x64 bk32 twin", (3, 104, 59, 58, 32, 3, 1, 1, 1), "d"),
    ("64x64", (3, 32, 59, 58, 192, 3, 1, 1, 1), "f"),
    ("64x64 twin", (3, 192, 59, 58, 32, 3, 1, 1, 1), "d"),
    ("64x256", (3, 16, 185, 187, 56, 3, 1, 1, 1), "f"),                 # 406 tiles of 256 pixels
    ("64x256 twin", (3, 56, 185, 187, 16, 3, 1, 1, 1), "d"),
    ("64x128 bk16", (3, 16, 13, 11, 40, 3, 1, 1, 1), "f"),
    ("64x128 bk16 twin", (3, 40, 13, 11, 16, 3, 1, 1, 1), "d"),
    ("64x128 bk32", (3, 32, 13, 11, 40, 3, 1, 1, 1), "f"),
    ("64x128 bk32 twin", (3, 40, 13, 11, 32, 3, 1, 1, 1), "d"),
    ("generic Cin=20", (2, 20, 19, 23, 104, 3, 1, 1, 1), "f"),
    ("generic Cin=20 twin", (2, 104, 19, 23, 24, 3, 1, 1, 1), "d"),     # (its K channels are the 24 of dY)
    ("generic Cout=30", (2, 16, 13, 11, 30, 1, 1, 0, 1), "f"),          # split kernels; generic under conv_split=0
    ("stem", (3, 3, 33, 71, 64, 7, 2, 3, 1), "f"),
    ("splitk vec4", (2, 64, 14, 18, 96, 3, 1, 1, 1), "f"),              # 8 tiles -> 4 K slices; OH*OW = 252
    ("splitk vec4 twin", (2, 96, 14, 18, 64, 3, 1, 1, 1), "d"),
    ("splitk plain", (2, 64, 13, 19, 96, 3, 1, 1, 1), "f"),             # OH*OW = 247
    ("splitk plain twin", (2, 96, 13, 19, 64, 3, 1, 1, 1), "d"),
    ("splitk bands", (2, 32, 19, 35, 72, 3, 1, 12, 12), "f"),           # two K slices AND the column bands [0,12) [12,23) [23,35)
    ("splitk bands twin", (2, 72, 19, 35, 32, 3, 1, 12, 12), "d"),
    ("3x3 stride 2", (2, 32, 19, 23, 64, 3, 2, 1, 1), "fd"),            # the sh=2 gather of the input gradient
    ("1x1 stride 2", (2, 48, 19, 23, 96, 1, 2, 0, 1), "fd"),
]
_BY_NAME = {n: (s, p) for n, s, p in RAGGED}
FWD_NAMES = [n for n, _s, p in RAGGED if "f" in p]
DGRAD_NAMES = [n for n, _s, p in RAGGED if "d" in p]

# what the table must have shown, as the trace names it: (description, regular expression on the configuration key,
# arithmetic label or None for any, passes it must have been seen in)
REQUIRED = [
    ("split<256,128,16> il=1", r"^split<256,128,16> ar=1 il=1 nsrc=0 ks=1 ", "fp16x2", "fd"),
    ("split<256,128,16> il=0 (conv_il=0)", r"^split<256,128,16> ar=1 il=0 ", PLAIN, "fd"),
    ("split<256,128,16> ks=2", r"^split<256,128,16> .* ks=2 ", None, "fd"),
    ("split<256,128,16> xcd_py != 0", r"^split<256,128,16> .* xcd_py=[1-9]", None, "fd"),
    ("split<256,128,16> nb>1", r"^split<256,128,16> .* nb=[2-9]", None, "fd"),
    ("split<128,128,16>", r"^split<128,128,16> ", None, "fd"),
    ("split<128,64,16>", r"^split<128,64,16> ", None, "fd"),
    ("split<128,64,32>", r"^split<128,64,32> ", None, "fd"),
    ("split<64,256,16>", r"^split<64,256,16> ", None, "fd"),
    ("split<64,128,16>", r"^split<64,128,16> ", None, "fd"),
    ("split<64,128,32>", r"^split<64,128,32> ", None, "fd"),
    ("split<64,64,32>", r"^split<64,64,32> ", None, "fd"),
    ("fp32_fast<128,128,16>", r"^fp32_fast<128,128,16> ", "fp32 MFMA", "fd"),
    ("fp32_fast<128,64,16>", r"^fp32_fast<128,64,16> ", "fp32 MFMA", "fd"),
    ("fp32_fast<128,64,32>", r"^fp32_fast<128,64,32> ", "fp32 MFMA", "fd"),
    ("fp32_fast<64,256,16>", r"^fp32_fast<64,256,16> ", "fp32 MFMA", "fd"),
    ("fp32_fast<64,128,16>", r"^fp32_fast<64,128,16> ", "fp32 MFMA", "fd"),
    ("fp32_fast<64,128,32>", r"^fp32_fast<64,128,32> ", "fp32 MFMA", "fd"),
    ("fp32_generic", r"^fp32_generic<", None, "fd"),
    ("the stem kernel", r"^stem7x7s2 ", None, "f"),
    ("split-K with splitk_reduce_vec4", r"ks=[2-9].*; splitk_reduce_vec4$", None, "fd"),
    ("split-K with plain splitk_reduce", r"ks=[2-9].*; splitk_reduce$", None, "fd"),
]

TERMS = [("none", ""), ("shift", "h"), ("scale+shift", "ch"), ("relu", "r"), ("residual", "e"), ("scale+shift+relu", "chr"),
         ("scale+shift+residual+relu", "cher")]
AMAX_PUBLISHERS = ["split epilogue", "splitk_reduce_vec4", "splitk_reduce", "stem", "read pass behind fp32"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _traced(ops):
    """The launch trace on; whatever the body did to the options is undone."""
    ops.launch_trace(True)
    try:
        yield
    finally:
        ops.launch_trace(False)
        set_options(ops, DEFAULTS)


def _sweep(ops, wd, passes, fn):
    """fn(label, pass, wt_fwd, wt_dgrad) -> launch trace, for every arithmetic of the full-size test's table and every pass it lists
    there; the plain loop (conv_il=0) only for the passes whose trace said il=1 under the default arithmetic."""
    il_seen = set()
    for label, opts, arith_passes in ARITHMETICS:
        if label == PLAIN and not il_seen:
            continue
        set_options(ops, opts)
        wf, wdg = ops.prep_weights(wd)
        for pas in passes:
            if pas not in arith_passes or (label == PLAIN and pas not in il_seen):
                continue
            trace = fn(label, pas, wf, wdg)
            if label == "fp16x2" and "il=1" in trace:
                il_seen.add(pas)


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # the inputs and float64 references this module kept on the device


def _make_case(dev, seed_name, shape, passes):
    """Inputs on the device and the float64 references of ``passes`` (computed once per process, never modified)."""
    from weaklysuperviseddl_amd import ops
    B, Cin, H, W, Cout, k, s, pad, d = shape
    g = torch.Generator().manual_seed(zlib.crc32(seed_name.encode()))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    OH, OW = ops.conv_out_hw(H, W, k, s, pad, d)
    dy = torch.randn(B, Cout, OH, OW, generator=g)
    c = dict(shape=shape, x=x.to(dev), w=w.to(dev), dy=dy.to(dev), g=g, ref={}, out_shape=(B, Cout, OH, OW))
    t0 = time.time()
    with cpu_threads(min(16, torch.get_num_threads())):
        x64, w64, dy64 = x.double(), w.double(), dy.double()
        if "f" in passes:
            c["ref"]["f"] = fwd64(x64, w64, s, pad, d).to(dev)
        if "d" in passes:
            c["ref"]["d"] = dgrad64(x.shape, w64, dy64, s, pad, d).to(dev)
        if "w" in passes:
            c["ref"]["w"] = wgrad64(x64, w.shape, dy64, s, pad, d).to(dev)
    c["host_s"] = time.time() - t0
    return c


def _case(dev, name):
    if name not in _CASES:
        shape, passes = _BY_NAME[name]
        _CASES[name] = _make_case(dev, name, shape, passes)
    return _CASES[name]


def _epilogue_terms(dev, c):
    """scale in [0.5, 1.5], shift and residual ~ N(0, 1) beside a raw convolution that is N(0, 1) itself: no term dwarfs another."""
    if "scale" not in c:
        _B, Cout = c["out_shape"][:2]
        g = c["g"]
        c["scale"] = (torch.rand(Cout, generator=g) + 0.5).to(dev)
        c["shift"] = torch.randn(Cout, generator=g).to(dev)
        c["res"] = torch.randn(c["out_shape"], generator=g).to(dev)
    return c["scale"], c["shift"], c["res"]


def _epilogue64(y64, scale, shift, res, terms):
    v = y64
    if "c" in terms:
        v = v * scale.double().view(1, -1, 1, 1)
    if "h" in terms:
        v = v + shift.double().view(1, -1, 1, 1)
    if "e" in terms:
        v = v + res.double()
    return v.clamp_min(0) if "r" in terms else v


def _fwd(ops, c, wf, terms="", **kw):
    _B, _Cin, _H, _W, _Cout, _k, s, pad, d = c["shape"]
    scale, shift, res = (c.get("scale"), c.get("shift"), kw.pop("residual", c.get("res")))
    return ops.conv2d_fwd(kw.pop("x", c["x"]), wf, c["w"].shape, s, pad, d, scale=scale if "c" in terms else None,
                          shift=shift if "h" in terms else None, residual=res if "e" in terms else None, relu="r" in terms, **kw)


# ------------------------------------------------------------------------------------------------------------- part 1
_RAGGED_TABLE = Table()
_RAGGED_DONE = {}
_T0 = [None]


def _run_ragged(ops, dev, name):
    if name in _RAGGED_DONE:
        return
    if _T0[0] is None:
        _T0[0] = time.time()
    c = _case(dev, name)
    B, Cin, H, W, Cout, k, s, pad, d = c["shape"]
    passes = _BY_NAME[name][1]

    def run(label, pas, wf, wdg):
        ops.last_launches()
        if pas == "f":
            out = ops.conv2d_fwd(c["x"], wf, c["w"].shape, s, pad, d)
        else:
            out = ops.conv2d_dgrad(c["dy"], wdg, c["w"].shape, c["x"].shape, s, pad, d)
        trace = ops.last_launches()
        err = pass_err(out, c["ref"][pas], pas)
        print(f"ragged {name!r} {PASS_NAME[pas]} {label}: {err:.3e}  {trace}")
        assert err <= TOL, (name, c["shape"], pas, label, err, trace)
        _RAGGED_TABLE.add(config_key(trace), PASS_NAME[pas], label, err, f"{name} B={B} {H}x{W}")
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], passes, run)
    _RAGGED_DONE[name] = True


@pytest.mark.parametrize("name", [n for n, _s, _p in RAGGED])
def test_ragged_shape_vs_float64(dev, name):
    from weaklysuperviseddl_amd import ops
    _run_ragged(ops, dev, name)


def test_ragged_table_reaches_every_configuration(dev):
    """The table above really runs what it was built for: every configuration of REQUIRED, forward and input gradient, is among
    the configuration keys the library's own trace gave.  A changed dispatch threshold fails here instead of silently emptying
    the table."""
    import re
    from weaklysuperviseddl_amd import ops
    for name, _s, _p in RAGGED:
        _run_ragged(ops, dev, name)
    torch.cuda.synchronize()
    _RAGGED_TABLE.report("ragged conv shapes in every forward / input-gradient configuration", time.time() - _T0[0])
    rows = list(_RAGGED_TABLE.rows)
    missing = []
    for what, pattern, arith, passes in REQUIRED:
        for pas in passes:
            if not any(re.search(pattern, key) and p == PASS_NAME[pas] and (arith is None or a == arith) for key, p, a in rows):
                missing.append((what, PASS_NAME[pas]))
    assert not missing, (missing, sorted({key for key, _p, _a in rows}))


# ------------------------------------------------------------------------------------------------------------- part 2
_EPI_TABLE = Table()
_EPI_DONE = {}
_AMAX_CHECKED = {p: 0 for p in AMAX_PUBLISHERS}


def _publisher(trace):
    if trace.startswith("stem"):
        return "stem"
    if trace.endswith("splitk_reduce_vec4"):
        return "splitk_reduce_vec4"
    if trace.endswith("splitk_reduce"):
        return "splitk_reduce"
    return "split epilogue" if trace.startswith("split<") else "read pass behind fp32"


def _run_epilogue(ops, dev, name):
    if name in _EPI_DONE:
        return
    c = _case(dev, name)
    B, _Cin, H, W = c["x"].shape
    scale, shift, res = _epilogue_terms(dev, c)
    is_stem = name == "stem"
    refs = {terms: _epilogue64(c["ref"]["f"], scale, shift, res, terms) for _t, terms in TERMS}

    def run(label, pas, wf, _wdg):
        for tname, terms in TERMS:
            ops.last_launches()
            out = _fwd(ops, c, wf, terms, want_amax=True)
            trace = ops.last_launches()
            err = chan_err(out, refs[terms], 1)
            print(f"epilogue {name!r} {label} [{tname}]: {err:.3e}  {trace}")
            assert err <= TOL, (name, label, tname, err, trace)
            if is_stem:
                # the stem kernel has no residual term: a residual must leave it (stem_eligible), and still be right
                assert ("stem" in trace) == ("e" not in terms), (tname, trace)
            _EPI_TABLE.add(config_key(trace), "fwd", label, err, f"{name} [{tname}]")
            top = out.abs().max().item()
            amax = getattr(out, "_wsdl_amax", None)
            if amax is not None:
                # the published amax is a maximum of the floats the kernel stored, not a new computation
                assert amax.item() == top, (name, label, tname, amax.item(), top, trace)
                _AMAX_CHECKED[_publisher(trace)] += 1
            if terms in ("chr", "cher"):
                # a caller's slot (the slices of one buffer share one): a larger value stays, a smaller one is raised to max|out|
                big = torch.full((1,), 3.0e30, device=dev)
                small = torch.full((1,), 1.0e-3, device=dev)
                _fwd(ops, c, wf, terms, y_amax=big)
                o2 = _fwd(ops, c, wf, terms, y_amax=small)
                assert torch.equal(o2, out), (name, label, tname)
                assert big.item() == torch.tensor(3.0e30).item(), (name, label, tname, big.item(), trace)
                assert small.item() == top, (name, label, tname, small.item(), top, trace)
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], "f", run)
    _EPI_DONE[name] = True


@pytest.mark.parametrize("name", FWD_NAMES)
def test_fused_epilogue_and_published_amax(dev, name):
    from weaklysuperviseddl_amd import ops
    _run_epilogue(ops, dev, name)


def test_every_amax_publisher_was_read_back(dev):
    from weaklysuperviseddl_amd import ops
    t0 = time.time()
    for name in FWD_NAMES:
        _run_epilogue(ops, dev, name)
    torch.cuda.synchronize()
    _EPI_TABLE.report("fused conv epilogue, seven term sets per configuration (worst of them)", time.time() - t0)
    report_line("    published amax == max|out| bit for bit: " + ", ".join(f"{k} x{v}" for k, v in _AMAX_CHECKED.items()))
    assert all(v > 0 for v in _AMAX_CHECKED.values()), _AMAX_CHECKED


# ------------------------------------------------------------------------------------------------------------- part 3
def _wide(dev, like, c0, extra, fill=None, g=None):
    """A tensor with ``extra`` more channels than ``like``'s shape -> (wide, its channel slice [c0, c0 + C))."""
    B, Cc, H, W = like
    if fill is None:
        wide = torch.randn(B, Cc + extra, H, W, generator=g).to(dev)
    else:
        wide = torch.full((B, Cc + extra, H, W), fill, device=dev)
    return wide, wide[:, c0:c0 + Cc]


SLICED_FWD = [
    # (RAGGED case or own shape, extra channels, first channel, plain split-K reduce expected)
    ("splitk vec4", None, 8, 4, "splitk_reduce_vec4"),        # H*W = 252: every batch stride a multiple of 4 floats
    ("splitk plain", None, 3, 1, "splitk_reduce"),            # H*W = 247, odd strides: the 16-byte reduce must not be chosen
    ("splitk plain", None, 4, 2, "splitk_reduce"),            # ... nor with strides that are multiples of 4, OH*OW being odd
    ("banded", (2, 16, 19, 35, 72, 3, 1, 12, 12), 3, 1, "nb=3"),          # H*W = 665; bands [0,12) [12,23) [23,35)
    ("banded", (2, 16, 19, 35, 72, 3, 1, 12, 12), 4, 2, "nb=3"),
    ("t256", None, 3, 1, "split<256,128,16>"),                # H*W = 5475
    ("t256", None, 4, 2, "split<256,128,16>"),
]
SENTINEL = -12345.0


@pytest.mark.parametrize("case", SLICED_FWD, ids=lambda cs: f"{cs[0]}+{cs[2]}")
def test_fwd_on_channel_slices(dev, case):
    """x, out and the residual are channel slices of wider tensors: the slice is right, nothing outside it is written, and the
    published amax is the slice's maximum (the wide output's sentinel is far larger)."""
    from weaklysuperviseddl_amd import ops
    name, shape, extra, c0, expect = case
    if shape is None:
        c = _case(dev, name)
    else:
        if name not in _CASES:
            _CASES[name] = _make_case(dev, name, shape, "f")
        c = _CASES[name]
    scale, shift, res = _epilogue_terms(dev, c)
    ref = _epilogue64(c["ref"]["f"], scale, shift, res, "cher")
    B, Cout, OH, OW = c["out_shape"]
    g = torch.Generator().manual_seed(7)
    xw, xs = _wide(dev, c["x"].shape, c0, extra, g=g)
    xs.copy_(c["x"])
    rw, rs = _wide(dev, c["out_shape"], c0, extra, g=g)
    rs.copy_(res)

    def run(label, pas, wf, _wdg):
        yw, ys = _wide(dev, c["out_shape"], c0, extra, fill=SENTINEL)
        ops.last_launches()
        out = _fwd(ops, c, wf, "cher", x=xs, residual=rs, out=ys, want_amax=True)
        trace = ops.last_launches()
        assert out.data_ptr() == ys.data_ptr()
        if not (expect.startswith("split<") and label == "fp32 MFMA"):
            assert expect in trace and (expect != "splitk_reduce" or trace.endswith(expect)), (expect, trace)
        err = chan_err(ys, ref, 1)
        print(f"sliced fwd {name!r}+{extra} {label}: {err:.3e}  strides x {xs.stride(0)} y {ys.stride(0)}  {trace}")
        assert err <= TOL, (name, extra, label, err, trace)
        assert (yw[:, :c0] == SENTINEL).all() and (yw[:, c0 + Cout:] == SENTINEL).all(), (name, extra, label, "wrote outside the slice")
        amax = getattr(out, "_wsdl_amax", None)
        if amax is not None:
            assert amax.item() == ys.abs().max().item(), (name, extra, label, amax.item(), ys.abs().max().item(), trace)
        slot = torch.full((1,), 1.0e-3, device=dev)
        _fwd(ops, c, wf, "cher", x=xs, residual=rs, out=ys, y_amax=slot)
        assert slot.item() == ys.abs().max().item(), (name, extra, label, slot.item(), trace)
        assert (yw[:, :c0] == SENTINEL).all() and (yw[:, c0 + Cout:] == SENTINEL).all()
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], "f", run)


SLICED_GRADS = [
    ("wgrad fp16x2 split", (3, 128, 9, 11, 256, 3, 1, 2, 2), "wgrad_split"),     # Cin and Cout multiples of 128
    ("wgrad fp32", (3, 32, 9, 11, 48, 3, 1, 1, 1), "wgrad"),
]


@pytest.mark.parametrize("case", SLICED_GRADS, ids=lambda cs: cs[0])
@pytest.mark.parametrize("extra,c0", [(3, 1), (4, 2)])
def test_dgrad_and_wgrad_on_channel_slices(dev, case, extra, c0):
    from weaklysuperviseddl_amd import ops
    name, shape, expect = case
    if name not in _CASES:
        _CASES[name] = _make_case(dev, name, shape, "dw")
    c = _CASES[name]
    _B, _Cin, _H, _W, _Cout, _k, s, pad, d = shape
    g = torch.Generator().manual_seed(11)
    _xw, xs = _wide(dev, c["x"].shape, c0, extra, g=g)
    xs.copy_(c["x"])
    _dw, dys = _wide(dev, c["out_shape"], c0, extra, g=g)
    dys.copy_(c["dy"])
    table = Table()
    t0 = time.time()

    def run(label, pas, _wf, wdg):
        ops.last_launches()
        if pas == "d":
            out = ops.conv2d_dgrad(dys, wdg, c["w"].shape, c["x"].shape, s, pad, d)
        else:
            out = ops.conv2d_wgrad(xs, dys, c["w"].shape, s, pad, d)
        trace = ops.last_launches()
        err = pass_err(out, c["ref"][pas], pas)
        print(f"sliced {name!r}+{extra} {PASS_NAME[pas]} {label}: {err:.3e}  {trace}")
        assert err <= TOL, (name, extra, pas, label, err, trace)
        if pas == "w" and label == "fp16x2":
            assert expect in trace, (expect, trace)
        table.add(config_key(trace), PASS_NAME[pas], label, err, f"{name}+{extra}")
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], "dw", run)
    table.report(f"dy / x as channel slices (+{extra} channels): {name}", time.time() - t0)


@pytest.mark.parametrize("name", DGRAD_NAMES)
def test_dgrad_accumulate_and_mask(dev, name):
    """dx = dgrad + previous against float64, and the masked form bit-identical to accumulating into previous * keep, in every
    input-gradient configuration of the ragged table."""
    from weaklysuperviseddl_amd import ops
    c = _case(dev, name)
    _B, _Cin, _H, _W, _Cout, _k, s, pad, d = c["shape"]
    xshape = tuple(c["x"].shape)
    assert c["x"].numel() % 8 == 0          # (every shape of the table was chosen so)
    g = torch.Generator().manual_seed(13)
    # the previous value at the gradient's own size: beside a unit-variance one the 16-channel twins' gradients (rms ~0.2) would
    # be a fifth of what the per-channel measure judges
    prev = torch.randn(xshape, generator=g) * c["ref"]["d"].std().item()
    keep = torch.rand(xshape, generator=g) < 0.5
    bits = torch.from_numpy(np.packbits(keep.numpy().reshape(-1), bitorder="little")).to(dev)
    prev_d, masked_d = prev.to(dev), (prev * keep).to(dev)
    ref = c["ref"]["d"] + prev_d.double()
    ref_masked = c["ref"]["d"] + masked_d.double()

    def run(label, pas, _wf, wdg):
        ops.last_launches()
        dx2 = ops.conv2d_dgrad(c["dy"], wdg, c["w"].shape, xshape, s, pad, d, accumulate_into=prev_d.clone())
        trace = ops.last_launches()
        err = chan_err(dx2, ref, 1)
        dx3 = ops.conv2d_dgrad(c["dy"], wdg, c["w"].shape, xshape, s, pad, d, accumulate_into=prev_d.clone(), acc_mask=bits)
        dx4 = ops.conv2d_dgrad(c["dy"], wdg, c["w"].shape, xshape, s, pad, d, accumulate_into=masked_d.clone())
        err_m = chan_err(dx3, ref_masked, 1)
        print(f"dgrad accumulate {name!r} {label}: {err:.3e} masked {err_m:.3e}  {trace}")
        assert err <= TOL and err_m <= TOL, (name, label, err, err_m, trace)
        assert torch.equal(dx3, dx4), (name, label, "masked accumulate", trace)
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], "d", run)


def test_fwd_group_on_a_non_square_banded_map(dev):
    """``conv2d_fwd_group`` on the smallest map ``fwd_group_ok`` admits with 256 output channels - B = 2, 20 x 24: 960 pixels are
    8 tiles of 128, the last one ragged - with dilations 8 and 12 (three and two column bands) and 24 (centre tap only)."""
    from weaklysuperviseddl_amd import ops
    B, C, H, W, Co = 2, 16, 20, 24, 256
    ks, dils = [1, 3, 3, 3], [1, 8, 12, 24]
    assert ops.fwd_group_ok(4, (B, C, H, W), Co)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, C, H, W, generator=g)
    ws = [torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5 for k in ks]
    with cpu_threads(min(16, torch.get_num_threads())):
        y64 = [fwd64(x.double(), w.double(), 1, d * (k - 1) // 2, d).to(dev) for w, k, d in zip(ws, ks, dils)]
    xd, wsd = x.to(dev), [w.to(dev) for w in ws]
    table = Table()
    t0 = time.time()
    with _traced(ops):
        for label, opts, _passes in ARITHMETICS:
            if label == "fp32 MFMA":
                continue                    # (the grouped entry point exists on the split kernels only)
            set_options(ops, opts)
            preps = [ops.prep_weights(w) for w in wsd]
            ops.last_launches()
            outs = ops.conv2d_fwd_group(xd, [p[0] for p in preps], [tuple(w.shape) for w in ws], dils)
            trace = ops.last_launches()
            assert "group split<256,128,16>" in trace, trace
            for i, (o, r) in enumerate(zip(outs, y64)):
                err = chan_err(o, r, 1)
                print(f"grouped forward {label} problem {i}: {err:.3e}  {trace}")
                assert err <= TOL, ("grouped forward", label, i, err, trace)
                table.add(config_key(trace), "fwd", label, err, f"k={ks[i]} d={dils[i]} B={B} {H}x{W}")
    table.report("grouped forward on a non-square banded map", time.time() - t0)


def test_dgrad_multi_on_a_non_square_banded_map(dev):
    """``conv2d_dgrad_multi`` with and without ``accumulate_into`` on the smallest non-square map ``dgrad_multi_ok`` admits for
    512 input channels (B = 3, 133 x 41: 128 pixel tiles, the last one ragged, an odd number of pixels per image); the first
    source's dilation 8 cuts the columns into the bands [0,8) [8,33) [33,41)."""
    from weaklysuperviseddl_amd import ops
    B, C, H, W, Co = 3, 512, 133, 41, 16
    ks, dils = [3, 3, 1], [8, 12, 1]
    assert ops.dgrad_multi_ok(3, (B, C, H, W), Co)
    assert not ops.dgrad_multi_ok(3, (B, C, H - 1, W), Co)          # one tile fewer is refused: this is the smallest
    g = torch.Generator().manual_seed(19)
    ws = [torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5 for k in ks]
    dys = [torch.randn(B, Co, H, W, generator=g) * sc for sc in (1.0, 0.25, 4.0)]
    prev = torch.randn(B, C, H, W, generator=g)
    t0 = time.time()
    with cpu_threads(min(16, torch.get_num_threads())):
        dx64 = sum(dgrad64((B, C, H, W), w.double(), dy.double(), 1, d * (k - 1) // 2, d) for w, dy, k, d in zip(ws, dys, ks, dils)).to(dev)
    host_s = time.time() - t0
    wsd, dysd, prev_d = [w.to(dev) for w in ws], [dy.to(dev) for dy in dys], (prev * dx64.std().item()).to(dev)      # at the gradient's size
    acc64 = dx64 + prev_d.double()
    table = Table()
    with _traced(ops):
        for label, opts, _passes in ARITHMETICS:
            if label == "fp32 MFMA":
                continue
            set_options(ops, opts)
            preps = [ops.prep_weights(w) for w in wsd]
            args = (dysd, [p[1] for p in preps], [tuple(w.shape) for w in ws], dils, (B, C, H, W))
            ops.last_launches()
            dx = ops.conv2d_dgrad_multi(*args)
            trace = ops.last_launches()
            assert "nsrc=2" in trace and "nb=3" in trace, trace
            dxa = ops.conv2d_dgrad_multi(*args, accumulate_into=prev_d.clone())
            err, err_a = chan_err(dx, dx64, 1), chan_err(dxa, acc64, 1)
            print(f"multi-source input gradient {label}: {err:.3e} accumulate {err_a:.3e}  {trace}")
            assert err <= TOL and err_a <= TOL, (label, err, err_a, trace)
            table.add(config_key(trace), "dgrad", label, max(err, err_a), f"3 sources B={B} {H}x{W}")
    table.report(f"multi-source input gradient on a non-square banded map (float64 host oracle {host_s:.0f} s)", time.time() - t0)


# ------------------------------------------------------------------------------------------------------------- part 4
# (name, k, stride, pad, dil, H, W)
GEOMETRIES = [
    ("3x3 pad 0", 3, 1, 0, 1, 17, 23),
    ("3x3 pad 2 (output larger than input)", 3, 1, 2, 1, 17, 23),
    ("3x3 stride 2 pad 0 even", 3, 2, 0, 1, 18, 22),
    ("3x3 stride 2 pad 1 even", 3, 2, 1, 1, 18, 22),
    ("3x3 stride 2 pad 0 odd", 3, 2, 0, 1, 17, 23),
    ("3x3 stride 2 pad 1 odd", 3, 2, 1, 1, 17, 23),
    ("3x3 stride 2 dil 2 pad 2", 3, 2, 2, 2, 19, 22),
    ("3x3 dil 3 pad 1 (pad < dil)", 3, 1, 1, 3, 17, 23),
    ("5x5 pad 2", 5, 1, 2, 1, 17, 23),
    ("5x5 pad 2 stride 2", 5, 2, 2, 1, 17, 23),
    ("1x1 stride 3", 1, 3, 0, 1, 17, 23),
    ("3x3 dil 12 pad 12, 9 rows", 3, 1, 12, 12, 9, 31),
    ("3x3 dil 12 pad 12, 9 columns", 3, 1, 12, 12, 31, 9),
]
CHANNELS = [("split-eligible", 32, 48), ("generic", 20, 30), ("split weight gradient", 128, 128)]


@pytest.mark.parametrize("chan", CHANNELS, ids=lambda ch: ch[0])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda gm: gm[0])
def test_geometry_outside_same_padding(dev, geom, chan):
    """Each geometry is either computed - all three passes within 1e-4 of float64 per channel - or refused with ``WsdlError``
    before anything is launched; never a wrong tensor.  Which of the two is recorded under "parity counts"."""
    from weaklysuperviseddl_amd import ops
    gname, k, s, pad, d, H, W = geom
    cname, Cin, Cout = chan
    B = 3
    name = f"{gname} / {cname}"
    if name not in _CASES:
        _CASES[name] = _make_case(dev, name, (B, Cin, H, W, Cout, k, s, pad, d), "fdw")
    c = _CASES[name]
    outcome = {}
    worst = [0.0]
    kernels = set()

    def run(label, pas, wf, wdg):
        ops.last_launches()
        try:
            if pas == "f":
                out = ops.conv2d_fwd(c["x"], wf, c["w"].shape, s, pad, d)
            elif pas == "d":
                out = ops.conv2d_dgrad(c["dy"], wdg, c["w"].shape, c["x"].shape, s, pad, d)
            else:
                out = ops.conv2d_wgrad(c["x"], c["dy"], c["w"].shape, s, pad, d)
        except ops.WsdlError as e:
            trace = ops.last_launches()
            assert trace == "", ("refused after a launch", name, pas, label, trace, str(e))
            outcome[(label, pas)] = "refused"
            return trace
        trace = ops.last_launches()
        err = pass_err(out, c["ref"][pas], pas)
        print(f"geometry {name!r} {PASS_NAME[pas]} {label}: {err:.3e}  {trace}")
        assert err <= TOL, (name, pas, label, err, trace)
        worst[0] = max(worst[0], err)
        kernels.add(config_key(trace).split(" ")[0])
        outcome[(label, pas)] = "computed"
        return trace

    with _traced(ops):
        _sweep(ops, c["w"], "fdw", run)
    kinds = set(outcome.values())
    assert len(kinds) == 1, (name, outcome)           # computed in every pass and arithmetic, or refused in every one
    if kinds == {"computed"}:
        report_line(f"conv geometry {name}: computed, {len(outcome)} (pass, arithmetic) runs, worst per-channel error {worst[0]:.2e} "
                    f"({', '.join(sorted(kernels))})")
    else:
        report_line(f"conv geometry {name}: refused with WsdlError before any launch")
