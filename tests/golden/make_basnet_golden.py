#!/usr/bin/env python3
"""Generate tests/golden/basnet.npz from the reference's own BASNet / RefUnet / BasicBlock bodies.

Runs ONLY where the reference checkout exists (like make_golden.py, whose ``lift`` it reuses).  ``models.resnet34`` is supplied
as a stand-in built from the lifted BasicBlock in ResNet-34's published layout (layer1..layer4 = BasicBlock x [3, 4, 6, 3], the
stride on conv1, a (1x1 conv, BN) downsample where the shape changes), so neither torchvision nor a download is needed.

Weights follow tests/basnet_oracle.py's rule per state_dict key.  The BatchNorm running statistics are calibrated with one
train-mode forward at momentum 1 on a calibration batch (without it, 16 residual blocks of eval-mode BatchNorm over arbitrary
statistics saturate every sigmoid) and stored.  The network then runs in eval mode in float64 on the fixture's cases.

    python tests/golden/make_basnet_golden.py         # rewrites tests/golden/basnet.npz
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF as _TRADITIONAL, lift  # noqa: E402
import basnet_oracle as bo  # noqa: E402

REF = os.path.join(os.path.dirname(_TRADITIONAL), "PretrainedBasnetModel", "model")


def resnet34_standin(BasicBlock):
    def resnet34(pretrained=False):
        net, inplanes = types.SimpleNamespace(), 64
        for li, (planes, n, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)), 1):
            down = None
            if stride != 1 or inplanes != planes:
                down = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes))
            blocks = [BasicBlock(inplanes, planes, stride, down)] + [BasicBlock(planes, planes) for _ in range(1, n)]
            setattr(net, f"layer{li}", nn.Sequential(*blocks))
            inplanes = planes
        return net
    return types.SimpleNamespace(resnet34=resnet34)


def build_reference():
    rn = lift(f"{REF}/resnet_model.py", {"conv3x3", "BasicBlock"})
    ns = lift(f"{REF}/BASNet.py", {"RefUnet", "BASNet"},
              {"models": resnet34_standin(rn["BasicBlock"]), "BasicBlock": rn["BasicBlock"]})
    return ns["BASNet"](3, 1)


def main():
    torch.set_num_threads(4)
    net = build_reference()
    keys_shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(bo.seeded_state_dict(keys_shapes))
    net = net.double()
    # calibration: one train-mode forward at momentum 1 (running statistics = the batch's)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 1.0
    calib = bo.input_batch(bo.input_u8(2, 128, 128, seed=7)).double()
    net.train()
    with torch.no_grad():
        net(calib)
    net.eval()
    sd = net.state_dict()
    stats = {k: v.float().numpy() if v.is_floating_point() else v.numpy()
             for k, v in sd.items() if "running_" in k or "num_batches_tracked" in k}
    out = {"keys": np.array([k for k, _ in keys_shapes]),
           "shapes": np.array(shape_rows(keys_shapes))}
    for k, v in stats.items():
        out["stat/" + k] = v
    # the stored float32 statistics are what the tests load: run the cases with exactly those
    net.load_state_dict(bo.seeded_state_dict(keys_shapes, stats))
    net = net.double().eval()
    for i, (B, H, W) in enumerate(bo.CASES):
        u8 = bo.input_u8(B, H, W, seed=100 + i)
        with torch.no_grad():
            ys = net(bo.input_batch(u8).double())
        out[f"case{i}/input_u8"] = u8
        out[f"case{i}/outputs"] = np.stack([y.numpy() for y in ys]).astype(np.float32)
        print(f"case {i} {B}x{H}x{W}: output ranges", [(round(float(y.min()), 3), round(float(y.max()), 3)) for y in ys])
    path = os.path.join(HERE, "basnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def shape_rows(keys_shapes):
    """shapes as a fixed-width int array: [ndim, d0, d1, d2, d3]"""
    return [[len(s)] + list(s) + [0] * (4 - len(s)) for _, s in keys_shapes]


if __name__ == "__main__":
    main()
