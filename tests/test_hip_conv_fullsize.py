"""Every convolution kernel configuration the BASELINE configs' training steps select, at the REAL geometry, against the
float64 oracle on the host.

The per-kernel tests (tests/test_hip_ops.py) compare against torch-CPU at sizes of at most ~100 tiles; the configurations the
benchmark spends its time in - the 256x128x16 form with its interleaved loop and XCD tile orders, the two-K-slice form of
layer3, the direct-fragment and LDS-staged fp16x2 weight gradients with their pixel splits, ASPP's grouped forward and
multi-source input gradient - are only chosen from >= 256 tiles on.  Here every unique convolution of DeepLabV3-ResNet50
(reached from /root/reference/TraditionalModel/SegmentationModel.py:102) runs forward, input gradient and
weight gradient at

    cfg2  B = 16, 256 x 256 input   (BASELINE configs[1]: 64 x 64 / 32 x 32 maps)
    cfg3  B = 32, 256 x 256 input   (configs[2])
    cfg5  B = 8,  512 x 512 input   (configs[4], one GPU's share: 128 x 128 / 64 x 64 maps)

in every arithmetic of the library (fp16x2 with the interleaved loop on and off, fp16x2 with the range guard, bf16x3,
exact-fp32 MFMA) and is compared with ``F.conv2d`` / ``torch.nn.grad.conv2d_input`` / ``conv2d_weight`` evaluated in FLOAT64 ON THE
HOST (1x1 convolutions as the three float64 matrix products they are - the host BLAS is several times faster than ATen's float64
convolution paths): max-norm error of every output channel relative to that channel's own maximum (rows AND columns of dW for the weight
gradient) - an error confined to one tile cannot hide in a tensor norm.  Bar: north_star's 1e-3; asserted 1e-4; measured ~1e-6.
Which configuration each comparison went through comes from the library itself (``wsdl_launch_trace``) and is printed with the
worst error per (configuration, pass, arithmetic) in the test summary ("parity counts").
"""
import re
import time

import pytest
import torch

from conv_oracle import ARITHMETICS, DEFAULTS, TOL, Table as _Table, chan_err as _chan_err, config_key as _config_key, \
    dgrad64 as _dgrad64, fwd64 as _fwd64, set_options as _set, wgrad64 as _wgrad64

pytestmark = pytest.mark.gpu

# (Cin, Cout, k, stride, dilation, input-map side at a 256 x 256 image, name, which passes)
SHAPES = [
    (3, 64, 7, 2, 1, 256, "conv1", "fw"),                      # (no input gradient: the image needs none)
    (64, 64, 1, 1, 1, 64, "l1.0.conv1", "fdw"),
    (64, 64, 3, 1, 1, 64, "l1.conv2", "fdw"),
    (64, 256, 1, 1, 1, 64, "l1.conv3/ds", "fdw"),
    (256, 64, 1, 1, 1, 64, "l1.conv1", "fdw"),
    (256, 128, 1, 1, 1, 64, "l2.0.conv1", "fdw"),
    (128, 128, 3, 2, 1, 64, "l2.0.conv2 s2", "fdw"),
    (128, 512, 1, 1, 1, 32, "l2.conv3", "fdw"),
    (256, 512, 1, 2, 1, 64, "l2.0.ds s2", "fdw"),
    (512, 128, 1, 1, 1, 32, "l2.conv1", "fdw"),
    (128, 128, 3, 1, 1, 32, "l2.conv2", "fdw"),
    (512, 256, 1, 1, 1, 32, "l3.0.conv1", "fdw"),
    (256, 256, 3, 1, 1, 32, "l3.0.conv2/head3x3", "fdw"),
    (256, 1024, 1, 1, 1, 32, "l3.conv3", "fdw"),
    (512, 1024, 1, 1, 1, 32, "l3.0.ds", "fdw"),
    (1024, 256, 1, 1, 1, 32, "l3.conv1", "fdw"),
    (256, 256, 3, 1, 2, 32, "l3.conv2 d2", "fdw"),
    (1024, 512, 1, 1, 1, 32, "l4.0.conv1", "fdw"),
    (512, 512, 3, 1, 2, 32, "l4.0.conv2 d2", "fdw"),
    (512, 2048, 1, 1, 1, 32, "l4.conv3", "fdw"),
    (1024, 2048, 1, 1, 1, 32, "l4.0.ds", "fdw"),
    (2048, 512, 1, 1, 1, 32, "l4.conv1", "fdw"),
    (512, 512, 3, 1, 4, 32, "l4.conv2 d4", "fdw"),
    (2048, 256, 1, 1, 1, 32, "aspp 1x1", "fdw"),
    (2048, 256, 3, 1, 12, 32, "aspp d12", "fdw"),
    (2048, 256, 3, 1, 24, 32, "aspp d24", "fdw"),
    (2048, 256, 3, 1, 36, 32, "aspp d36", "fdw"),
    (1280, 256, 1, 1, 1, 32, "aspp project", "fdw"),
    (1024, 256, 3, 1, 1, 32, "aux 3x3", "fdw"),
    (256, 2, 1, 1, 1, 32, "classifier.4", "fdw"),
    (256, 21, 1, 1, 1, 32, "aux_classifier.4", "fdw"),
]
CONFIGS = {"cfg2": (16, 1), "cfg3": (32, 1), "cfg5": (8, 2)}          # batch, scale of the 256 x 256 image


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_VERIFIED = set()       # (configuration, pass, map side, layer): compared with float64 at another batch size already in this process


def _run_shape(ops, dev, table, B, scale, shape, g, timing):
    Cin, Cout, k, s, d, H0, name, passes = shape
    H = H0 * scale
    pad = (k // 2) * d if k > 1 else 0
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    # Which configurations does this shape select at this batch size?  (The device side costs milliseconds; the float64
    # reference on the host is what this test's time goes into.)  A shape whose three passes run, at this map size, exactly
    # the configurations already compared at another batch size is not compared again: cfg3 repeats most of cfg2's.
    _set(ops, DEFAULTS)
    xd0, wd0 = x.to(dev), w.to(dev)
    wf0, wdg0 = ops.prep_weights(wd0)
    ops.last_launches()
    y0 = ops.conv2d_fwd(xd0, wf0, w.shape, s, pad, d)
    keys = [(_config_key(ops.last_launches()), "f", H, name)]
    if "d" in passes:
        ops.conv2d_dgrad(y0, wdg0, w.shape, x.shape, s, pad, d)
        keys.append((_config_key(ops.last_launches()), "d", H, name))
    ops.conv2d_wgrad(xd0, y0, w.shape, s, pad, d)
    keys.append((_config_key(ops.last_launches()), "w", H, name))
    del xd0, wd0, wf0, wdg0, y0
    if all(kk in _VERIFIED for kk in keys):
        timing["skipped"] += 1
        return
    _VERIFIED.update(keys)
    t_ref = time.time()
    x64, w64 = x.double(), w.double()
    # (1x1 convolutions as the three float64 matrix products they are: conv_oracle.py)
    y64 = _fwd64(x64, w64, s, pad, d)
    dy = torch.randn(y64.shape, generator=g)
    dy64 = dy.double()
    ref = {"f": y64.to(dev)}
    if "d" in passes:
        ref["d"] = _dgrad64(x.shape, w64, dy64, s, pad, d).to(dev)
    ref["w"] = _wgrad64(x64, w.shape, dy64, s, pad, d).to(dev)
    del x64, w64, y64, dy64
    timing["host_oracle_s"] += time.time() - t_ref
    xd, wd_, dyd = x.to(dev), w.to(dev), dy.to(dev)
    il_seen = {"f": False, "d": False}
    for label, opts, arith_passes in ARITHMETICS:
        if label == "fp16x2 plain loop" and not (il_seen["f"] or il_seen["d"]):
            continue
        _set(ops, opts)
        wf, wdg = ops.prep_weights(wd_)
        for pas in "fdw":
            if pas not in passes or pas not in arith_passes:
                continue
            if label == "fp16x2 plain loop" and not il_seen[pas]:
                continue
            ops.last_launches()
            if pas == "f":
                out = ops.conv2d_fwd(xd, wf, w.shape, s, pad, d)
            elif pas == "d":
                out = ops.conv2d_dgrad(dyd, wdg, w.shape, x.shape, s, pad, d)
            else:
                out = ops.conv2d_wgrad(xd, dyd, w.shape, s, pad, d)
            trace = ops.last_launches()
            if label == "fp16x2" and pas in il_seen and "il=1" in trace:
                il_seen[pas] = True
            errs = [_chan_err(out, ref[pas], 1 if pas != "w" else 0)]
            if pas == "w":
                errs.append(_chan_err(out, ref[pas], 1))
            err = max(errs)
            assert err <= TOL, (name, B, H, pas, label, err, trace)
            table.add(_config_key(trace), {"f": "fwd", "d": "dgrad", "w": "wgrad"}[pas], label, err, f"{name} B={B} {H}x{H}")
    _set(ops, DEFAULTS)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_conv_configuration_of_the_step_vs_float64_at_full_size(dev, cfg):
    from weaklysuperviseddl_amd import ops
    B, scale = CONFIGS[cfg]
    table = _Table()
    g = torch.Generator().manual_seed(1000 + B)
    t0 = time.time()
    timing = {"host_oracle_s": 0.0, "skipped": 0}
    ops.launch_trace(True)
    try:
        for shape in SHAPES:
            _run_shape(ops, dev, table, B, scale, shape, g, timing)
    finally:
        ops.launch_trace(False)
        _set(ops, DEFAULTS)
    torch.cuda.synchronize()
    table.report(f"conv configurations at {cfg} size (B={B}, {256 * scale} x {256 * scale}; float64 host oracle {timing['host_oracle_s']:.0f} s"
                 f"{', %d shapes already compared under the same configurations at another batch size' % timing['skipped'] if timing['skipped'] else ''})",
                 time.time() - t0)
    keys = {k for k, _p, _a in table.rows}
    # the configurations this test exists for are really reached at this size (cfg3 only adds what cfg2 has not shown)
    if cfg != "cfg3":
        assert any("split<256,128,16>" in k and "il=1" in k for k in keys), keys
        assert any("wgrad_split16d" in k for k in keys) and any(re.search(r"wgrad_split16 ", k) for k in keys), keys
    if cfg == "cfg2":
        assert any("split<256,128,16>" in k and "ks=2" in k for k in keys), keys       # layer3's two-K-slice form
        assert any("xcd_py=" in k and "xcd_py=0" not in k for k in keys), keys           # an XCD-aware tile order


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_aspp_grouped_forward_and_multi_source_dgrad_vs_float64_at_full_size(dev, cfg):
    """ASPP's four branch convolutions as ONE grouped forward launch and their input gradients as ONE multi-source launch
    (wsdl_conv2d_fwd_group / wsdl_conv2d_dgrad_multi), whole tensors against float64 on the host, per channel."""
    from weaklysuperviseddl_amd import ops
    B, scale = CONFIGS[cfg]
    H, C, Co = 32 * scale, 2048, 256
    ks, dils = [1, 3, 3, 3], [1, 12, 24, 36]
    g = torch.Generator().manual_seed(2000 + B)
    x = torch.randn(B, C, H, H, generator=g)
    ws = [torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5 for k in ks]
    dys = [torch.randn(B, Co, H, H, generator=g) * sc for sc in (1.0, 0.25, 4.0, 0.5)]
    x64 = x.double()
    t0 = time.time()
    def fwd64(w, k, d):
        return _fwd64(x64, w.double(), 1, d * (k - 1) // 2, d)

    def dgrad64(w, dy, k, d):
        return _dgrad64(x.shape, w.double(), dy.double(), 1, d * (k - 1) // 2, d)

    y64 = [fwd64(w, k, d).to(dev) for w, k, d in zip(ws, ks, dils)]
    dx64 = sum(dgrad64(w, dy, k, d) for w, dy, k, d in zip(ws, dys, ks, dils)).to(dev)
    del x64
    xd, wsd, dysd = x.to(dev), [w.to(dev) for w in ws], [dy.to(dev) for dy in dys]
    if not (ops.fwd_group_ok(4, tuple(x.shape), Co) and ops.dgrad_multi_ok(4, tuple(x.shape), Co)):
        pytest.skip("geometry not served by the grouped / multi-source kernels")
    table = _Table()
    ops.launch_trace(True)
    try:
        for label, opts, _passes in ARITHMETICS:
            if label == "fp32 MFMA":
                continue                    # (the grouped / multi-source entry points exist on the split kernels only)
            _set(ops, opts)
            preps = [ops.prep_weights(w) for w in wsd]
            ops.last_launches()
            outs = ops.conv2d_fwd_group(xd, [p[0] for p in preps], [tuple(w.shape) for w in ws], dils)
            trace = ops.last_launches()
            for i, (o, r) in enumerate(zip(outs, y64)):
                err = _chan_err(o, r, 1)
                assert err <= TOL, ("grouped forward", cfg, label, i, err, trace)
                table.add(_config_key(trace), "fwd", label, err, f"aspp branch {i} B={B} {H}x{H}")
            order = [1, 2, 3, 0]            # smallest dilation first (it decides the column bands)
            ops.last_launches()
            dx = ops.conv2d_dgrad_multi([dysd[i] for i in order], [preps[i][1] for i in order], [tuple(ws[i].shape) for i in order],
                                        [dils[i] for i in order], tuple(x.shape))
            trace = ops.last_launches()
            err = _chan_err(dx, dx64, 1)
            assert err <= TOL, ("multi-source input gradient", cfg, label, err, trace)
            table.add(_config_key(trace), "dgrad", label, err, f"aspp 4 sources B={B} {H}x{H}")
    finally:
        ops.launch_trace(False)
        _set(ops, DEFAULTS)
    torch.cuda.synchronize()
    table.report(f"ASPP grouped forward / multi-source input gradient at {cfg} size", time.time() - t0)
    assert any("group split<256,128,16>" in k for k, _p, _a in table.rows)
    assert any("nsrc=3" in k for k, _p, _a in table.rows)
