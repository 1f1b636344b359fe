"""What the float64 convolution parity tests share (tests/test_hip_conv_fullsize.py, tests/test_hip_conv_edges.py): the
float64 host references, the per-channel error measure, the arithmetics every case runs in, the kernel-configuration key read
from the library's launch trace and the (configuration, pass, arithmetic) table printed under "parity counts"."""
import re

import torch
import torch.nn.functional as F

from conftest import report_line

TOL = 1e-4          # north_star: 1e-3 relative; the kernels measure ~1e-6

# (label, library options, passes it applies to)
ARITHMETICS = [
    ("fp16x2", dict(conv_split=1, wgrad_split=1, conv_arith=1, conv_il=1), "fdw"),
    ("fp16x2 plain loop", dict(conv_split=1, wgrad_split=1, conv_arith=1, conv_il=0), "fd"),     # only where the trace says il=1
    ("fp16x2s (guard)", dict(conv_split=1, wgrad_split=1, conv_arith=2, conv_il=1), "fd"),
    ("bf16x3", dict(conv_split=1, wgrad_split=1, conv_arith=0, conv_il=1), "fdw"),
    ("fp32 MFMA", dict(conv_split=0, wgrad_split=0, conv_arith=1, conv_il=1), "fdw"),
]
DEFAULTS = dict(conv_split=1, wgrad_split=1, conv_arith=1, conv_il=1)
PASS_NAME = {"f": "fwd", "d": "dgrad", "w": "wgrad"}


def set_options(ops, opts):
    for k, v in opts.items():
        ops.set_option(k, v)


def chan_err(got, ref64, dim):
    """max over the other dims of |got - ref| per index of ``dim``, relative to that slice's own max |ref| -> worst slice."""
    dims = [d for d in range(ref64.dim()) if d != dim]
    diff = (got.double() - ref64).abs().amax(dim=dims)
    mag = ref64.abs().amax(dim=dims)
    top = mag.max()
    # a slice that is all (or nearly) zero - a dead tap's column of dW - is judged against the tensor's maximum
    return (diff / torch.maximum(mag, 1e-6 * top)).max().item()


def pass_err(got, ref64, pas):
    """``chan_err`` as each pass is judged: output channels of y / dx, rows AND columns of dW."""
    if pas == "w":
        return max(chan_err(got, ref64, 0), chan_err(got, ref64, 1))
    return chan_err(got, ref64, 1)


def config_key(trace):
    """The launch descriptions without their grid extents: the kernel configuration."""
    return re.sub(r" (grid|workgroups)=[0-9x]+", "", trace)


def fwd64(x64, w64, stride, pad, dil):
    """y in float64 on the host.  A 1x1 convolution is a matrix product per image (the float64 GEMM of the host's BLAS is
    several times faster than ATen's float64 convolution paths): y[b] = W x[b] on the strided pixels."""
    Cout, Cin, k, _ = w64.shape
    if k == 1 and pad == 0:
        xs = x64[:, :, ::stride, ::stride].contiguous()
        B, _, OH, OW = xs.shape
        return torch.matmul(w64.view(Cout, Cin), xs.view(B, Cin, OH * OW)).view(B, Cout, OH, OW)
    return F.conv2d(x64, w64, None, stride, pad, dil)


def dgrad64(xshape, w64, dy64, stride, pad, dil):
    """dx in float64 on the host: dx[b] = W^T dy[b] scattered to the strided pixels for a 1x1 convolution."""
    Cout, Cin, k, _ = w64.shape
    if k == 1 and pad == 0:
        B, _, OH, OW = dy64.shape
        dxs = torch.matmul(w64.view(Cout, Cin).t(), dy64.reshape(B, Cout, OH * OW)).view(B, Cin, OH, OW)
        dx = torch.zeros(xshape, dtype=torch.float64)
        dx[:, :, ::stride, ::stride] = dxs
        return dx
    return torch.nn.grad.conv2d_input(xshape, w64, dy64, stride, pad, dil)


def wgrad64(x64, wshape, dy64, stride, pad, dil):
    """dW in float64 on the host: dW = sum_b dy[b] x[b]^T over the strided pixels for a 1x1 convolution."""
    Cout, Cin, k, _ = wshape
    if k == 1 and pad == 0:
        xs = x64[:, :, ::stride, ::stride].contiguous()
        B, _, OH, OW = xs.shape
        return torch.einsum("bop,bip->oi", dy64.reshape(B, Cout, OH * OW), xs.view(B, Cin, OH * OW)).view(Cout, Cin, 1, 1)
    return torch.nn.grad.conv2d_weight(x64, wshape, dy64, stride, pad, dil)


class Table:
    def __init__(self):
        self.rows = {}          # (config key, pass, arithmetic) -> [worst error, example shape, count]

    def add(self, key, pas, arith, err, example):
        r = self.rows.setdefault((key, pas, arith), [0.0, example, 0])
        if err >= r[0]:
            r[0], r[1] = err, example
        r[2] += 1

    def report(self, title, seconds):
        report_line(f"{title}: {len(self.rows)} (kernel configuration, pass, arithmetic) combinations against the float64 host oracle "
                    f"in {seconds:.0f} s; worst per-channel max-norm error {max(r[0] for r in self.rows.values()):.2e}")
        for (key, pas, arith), (err, ex, n) in sorted(self.rows.items(), key=lambda kv: (kv[0][1], kv[0][0], kv[0][2])):
            report_line(f"    {pas:5s} {arith:18s} {err:.2e}  x{n:<2d} e.g. {ex:22s} {key}")
