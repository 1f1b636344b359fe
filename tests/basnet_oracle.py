"""BASNet's eval-mode forward restated functionally in torch-CPU float64 from a state_dict (reference
PretrainedBasnetModel/model/BASNet.py, ResNet-34 BasicBlock), and the deterministic weight rule the BASNet tests and
tests/golden/make_basnet_golden.py share.

Written from the network's published structure with F.conv2d / F.max_pool2d(ceil_mode=True) / F.interpolate; it is pinned to
the reference's own module bodies by tests/golden/basnet.npz (tests/test_basnet.py).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(1, 3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(1, 3, 1, 1)
CASES = ((2, 64, 64), (1, 96, 128))          # (B, H, W) of the fixture's inputs


def seeded_param(key, shape):
    """The value of a conv / BN parameter under the tests' rule (rng seeded by crc32 of the state_dict key):
    conv weights He-normal (fan-in), conv biases U(-0.1, 0.1), BN gamma 1 + N(0, 0.1^2), BN beta N(0, 0.1^2)."""
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    if len(shape) == 4:
        fan_in = shape[1] * shape[2] * shape[3]
        v = rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)
    elif key.endswith(".bias") and _is_conv_bias(key):
        v = rng.uniform(-0.1, 0.1, shape)
    elif key.endswith(".weight"):
        v = 1.0 + 0.1 * rng.standard_normal(shape)
    else:
        v = 0.1 * rng.standard_normal(shape)
    return torch.from_numpy(np.asarray(v, dtype=np.float32))


def _is_conv_bias(key):
    last = key.rsplit(".", 2)[-2]
    return last.startswith(("conv", "inconv", "outconv"))


def seeded_state_dict(keys_shapes, stats=None):
    """{key: tensor} for the reference's (key, shape) list: parameters by ``seeded_param``, running statistics and
    num_batches_tracked from ``stats`` (the fixture's calibrated values) or the BatchNorm defaults."""
    sd = {}
    for key, shape in keys_shapes:
        shape = tuple(int(s) for s in shape)
        if stats is not None and key in stats:
            sd[key] = torch.as_tensor(np.asarray(stats[key])).reshape(shape).clone()
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(0, dtype=torch.long)
        elif key.endswith("running_mean"):
            sd[key] = torch.zeros(shape)
        elif key.endswith("running_var"):
            sd[key] = torch.ones(shape)
        else:
            sd[key] = seeded_param(key, shape)
    return sd


def input_batch(u8):
    """(B,3,H,W) uint8 -> the network input: x / 255, ImageNet normalised, in float32."""
    x = u8.astype(np.float32) / np.float32(255.0)
    return torch.from_numpy((x - MEAN) / STD)


def input_u8(B, H, W, seed):
    """Smooth RGB test images as uint8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W] / max(H, W)
    img = np.zeros((B, 3, H, W))
    for b in range(B):
        for c in range(3):
            for _ in range(3):
                fy, fx, ph = rng.uniform(0, 3), rng.uniform(0, 3), rng.uniform(0, 6.28)
                img[b, c] += 0.25 * np.sin(6.28 * (fy * yy + fx * xx) + ph)
    img = 0.5 + 0.5 * img + 0.03 * rng.standard_normal(img.shape)
    return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the forward
def _conv(x, sd, name, stride=1, pad=1, dil=1):
    b = sd.get(name + ".bias")
    return F.conv2d(x, sd[name + ".weight"], b, stride=stride, padding=pad, dilation=dil)


def _bn(x, sd, name, eps=1e-5):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        False, 0.0, eps)


def _cbr(x, sd, conv, bn, pad=1, dil=1):
    return F.relu(_bn(_conv(x, sd, conv, pad=pad, dil=dil), sd, bn))


def _block(x, sd, p, stride=1):
    out = F.relu(_bn(_conv(x, sd, p + ".conv1", stride=stride), sd, p + ".bn1"))
    out = _bn(_conv(out, sd, p + ".conv2"), sd, p + ".bn2")
    idt = x
    if p + ".downsample.0.weight" in sd:
        idt = _bn(_conv(x, sd, p + ".downsample.0", stride=stride, pad=0), sd, p + ".downsample.1")
    return F.relu(out + idt)


def _pool(x):
    return F.max_pool2d(x, 2, 2, ceil_mode=True)


def _up(x, s):
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)


def refunet(x, sd, p="refunet."):
    hx = _conv(x, sd, p + "conv0")
    skips = []
    for i in range(1, 5):
        h = _cbr(hx, sd, f"{p}conv{i}", f"{p}bn{i}")
        skips.append(h)
        hx = _pool(h)
    d = _cbr(hx, sd, p + "conv5", p + "bn5")
    for i in (4, 3, 2, 1):
        d = _cbr(torch.cat((_up(d, 2), skips[i - 1]), 1), sd, f"{p}conv_d{i}", f"{p}bn_d{i}")
    return x + _conv(d, sd, p + "conv_d0")


def forward(sd, x):
    """-> the 8 outputs (sigmoid(dout), sigmoid(d1), ..., sigmoid(d6), sigmoid(db)) in float64."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.double()
    hx = _cbr(x, sd, "inconv", "inbn")
    hs = []
    for e, (n, stride) in enumerate(((3, 1), (4, 2), (6, 2), (3, 2)), 1):
        for i in range(n):
            hx = _block(hx, sd, f"encoder{e}.{i}", stride if i == 0 else 1)
        hs.append(hx)
    for s in (5, 6):
        hx = _pool(hx)
        for i in (1, 2, 3):
            hx = _block(hx, sd, f"resb{s}_{i}")
        hs.append(hx)
    h1, h2, h3, h4, h5, h6 = hs
    hx = _cbr(h6, sd, "convbg_1", "bnbg_1", 2, 2)
    hx = _cbr(hx, sd, "convbg_m", "bnbg_m", 2, 2)
    hbg = _cbr(hx, sd, "convbg_2", "bnbg_2", 2, 2)
    hd, prev = {}, hbg
    for s, skip in ((6, h6), (5, h5), (4, h4), (3, h3), (2, h2), (1, h1)):
        dil = 2 if s == 6 else 1
        hx = torch.cat((prev if s == 6 else _up(prev, 2), skip), 1)
        hx = _cbr(hx, sd, f"conv{s}d_1", f"bn{s}d_1")
        hx = _cbr(hx, sd, f"conv{s}d_m", f"bn{s}d_m", dil, dil)
        prev = hd[s] = _cbr(hx, sd, f"conv{s}d_2", f"bn{s}d_2", dil, dil)
    db = _up(_conv(hbg, sd, "outconvb"), 32)
    d = {s: _conv(hd[s], sd, f"outconv{s}") for s in range(1, 7)}
    scale = {6: 32, 5: 16, 4: 8, 3: 4, 2: 2}
    for s, f in scale.items():
        d[s] = _up(d[s], f)
    dout = refunet(d[1], sd)
    return tuple(torch.sigmoid(t) for t in (dout, d[1], d[2], d[3], d[4], d[5], d[6], db))
