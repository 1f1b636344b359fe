"""BASNet (reference PretrainedBasnetModel/model/BASNet.py, resnet_model.py BasicBlock) for eval-mode inference on the device.

The modules hold the reference's parameters under the reference's names, so ``net.load_state_dict(torch.load('basnet.pth'))``
works with ``strict=True``.  ResNet-34's layer1..layer4 are built here (BasicBlock x [3, 4, 6, 3], the stride on conv1, a
(1x1 conv, BN) downsample where the shape changes) instead of from ``torchvision.models.resnet34(pretrained=True)``: nothing is
imported from torchvision and nothing is downloaded.

The forward calls ``ops`` directly (no autograd, no saved activations):
  - every conv + BN pair is one ``conv2d_fwd`` with BN folded into scale / shift (``bn_fold_bias`` where the conv carries a
    bias) and the ReLU / residual in the epilogue; folded tensors and weight layouts are cached per parameter version;
  - each decoder stage's torch.cat((up, skip), 1) is one buffer: the encoder writes the skip into its second channel half,
    the x2 up-sample of the previous stage writes the first half.  Both producers publish their amax into one shared slot,
    which bounds the whole buffer (the up-sample is a convex combination of its input);
  - the 2x2 ceil-mode pools, side outputs, RefUnet tail and sigmoids are csrc/basnet.hip.
Inference only: a train-mode forward, a host tensor or a side that is not a multiple of 32 raise ``WsdlError``.
"""
import torch
import torch.nn as nn

from ... import ops
from ..._lib import WsdlError
from ...nn import BatchNorm2d, Conv2d

__all__ = ["BASNet", "RefUnet", "BasicBlock", "resnet34_layers"]


def _conv(x, conv, bn=None, relu=False, residual=None, out=None, y_amax=None):
    """relu(bn(conv(x)) + residual) in one conv2d_fwd; conv(x) + bias without ``bn``."""
    cache = conv.__dict__.setdefault("_wsdl_cache", {})
    wf, _ = ops._cached_prep(cache, conv.weight, False)
    if bn is not None:
        parts = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if conv.bias is not None:
            parts = parts + (conv.bias,)
        key = ops._cache_key(*parts)
        if cache.get("fold_key") != key:
            g, b = bn.weight.detach(), bn.bias.detach()
            if conv.bias is None:
                fold = ops.bn_fold(g, b, bn.running_mean, bn.running_var, bn.eps)
            else:
                fold = ops.bn_fold_bias(g, b, bn.running_mean, bn.running_var, conv.bias.detach(), bn.eps)
            cache["fold_key"], cache["fold"] = key, fold
        scale, shift = cache["fold"]
    else:
        scale, shift = None, (conv.bias.detach() if conv.bias is not None else None)
    return ops.conv2d_fwd(x, wf, tuple(conv.weight.shape), conv.stride, conv.padding, conv.dilation, scale, shift, residual,
                          relu, out=out, want_amax=True, y_amax=y_amax)


def _stage_buffer(B, C, H, W, device):
    """A decoder stage's concatenated input (B, 2C, H, W) and the amax slot its two halves' producers share."""
    buf = torch.empty(B, 2 * C, H, W, device=device, dtype=torch.float32)
    slot = ops.amax_slot(device)
    ops._publish_amax(buf, slot)
    return buf, slot


def _up_into(x, buf):
    """upscore2(x) into the first channel half of ``buf``."""
    ops.bilinear_into(x, buf[:, :x.shape[1]])


class BasicBlock(nn.Module):
    """ResNet BasicBlock (resnet_model.py): conv3x3 (no bias) -> BN -> ReLU -> conv3x3 -> BN, + identity / downsample, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride=stride, padding=1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, padding=1)
        self.bn2 = BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def run(self, x, out=None, y_amax=None):
        t = _conv(x, self.conv1, self.bn1, relu=True)
        ds = self.downsample
        idt = _conv(x, ds[0], ds[1]) if ds is not None else x
        return _conv(t, self.conv2, self.bn2, relu=True, residual=idt, out=out, y_amax=y_amax)

    def forward(self, x):
        _check_eval(self, x)
        return self.run(x)


def _run_layer(layer, x, out=None, y_amax=None):
    blocks = list(layer)
    for blk in blocks[:-1]:
        x = blk.run(x)
    return blocks[-1].run(x, out=out, y_amax=y_amax)


def resnet34_layers():
    """torchvision ResNet-34's layer1..layer4 (BasicBlock x [3, 4, 6, 3]) with its module names."""
    layers, inplanes = [], 64
    for planes, n, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        down = None
        if stride != 1 or inplanes != planes:
            down = nn.Sequential(Conv2d(inplanes, planes, 1, stride=stride), BatchNorm2d(planes))
        mods = [BasicBlock(inplanes, planes, stride, down)] + [BasicBlock(planes, planes) for _ in range(1, n)]
        layers.append(nn.Sequential(*mods))
        inplanes = planes
    return layers


def _check_eval(module, x):
    if any(m.training for m in module.modules()):
        raise WsdlError(f"{type(module).__name__}: inference only - call .eval() first (the reference never trains BASNet)")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise WsdlError(f"{type(module).__name__}: the HIP path needs a device tensor; there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise WsdlError(f"{type(module).__name__}: expected a (B,C,H,W) float32 tensor, got {tuple(x.shape)} {x.dtype}")


class RefUnet(nn.Module):
    """BASNet's residual refinement module (BASNet.py:9-102): forward(x) = x + conv_d0(decoder(encoder(conv0(x))))."""

    def __init__(self, in_ch, inc_ch):
        super().__init__()
        self.conv0 = Conv2d(in_ch, inc_ch, 3, padding=1, bias=True)
        chans = [inc_ch, 64, 64, 64, 64, 64]
        for i in range(1, 6):
            setattr(self, f"conv{i}", Conv2d(chans[i - 1], 64, 3, padding=1, bias=True))
            setattr(self, f"bn{i}", BatchNorm2d(64))
        for i in (4, 3, 2, 1):
            setattr(self, f"conv_d{i}", Conv2d(128, 64, 3, padding=1, bias=True))
            setattr(self, f"bn_d{i}", BatchNorm2d(64))
        self.conv_d0 = Conv2d(64, 1, 3, padding=1, bias=True)

    def run(self, x, out=None):
        """(sigmoid(x + residual) into ``out`` (or a new tensor), the logits x + residual)."""
        B, _, H, W = x.shape
        hx = _conv(x, self.conv0)
        bufs = []
        for i in range(1, 5):                        # hx_i into the second half of decoder stage i's input
            buf, slot = _stage_buffer(B, 64, hx.shape[2], hx.shape[3], x.device)
            hx_i = _conv(hx, getattr(self, f"conv{i}"), getattr(self, f"bn{i}"), relu=True, out=buf[:, 64:], y_amax=slot)
            hx = ops.max_pool_2x2_ceil(hx_i)
            bufs.append((buf, slot))
        buf, slot = bufs[3]
        d = _conv(hx, self.conv5, self.bn5, relu=True, y_amax=slot)
        for i in (4, 3, 2, 1):
            buf, _ = bufs[i - 1]
            _up_into(d, buf)
            d = _conv(buf, getattr(self, f"conv_d{i}"), getattr(self, f"bn_d{i}"), relu=True,
                      y_amax=bufs[i - 2][1] if i > 1 else None)
        return ops.side_output(d, self.conv_d0.weight, self.conv_d0.bias, 1, residual=x, out=out)

    def forward(self, x):
        _check_eval(self, x)
        return self.run(x)[1]


class BASNet(nn.Module):
    """BASNet(n_channels, n_classes) with the reference's parameter names; ``n_classes`` is accepted and unused, as there."""

    def __init__(self, n_channels, n_classes):
        super().__init__()
        self.inconv = Conv2d(n_channels, 64, 3, padding=1, bias=True)
        self.inbn = BatchNorm2d(64)
        self.encoder1, self.encoder2, self.encoder3, self.encoder4 = resnet34_layers()
        for s in (5, 6):
            for i in (1, 2, 3):
                setattr(self, f"resb{s}_{i}", BasicBlock(512, 512))
        for n in ("1", "m", "2"):
            setattr(self, f"convbg_{n}", Conv2d(512, 512, 3, padding=2, dilation=2, bias=True))
            setattr(self, f"bnbg_{n}", BatchNorm2d(512))
        # (stage, in of _1, out of _m, out of _2, dilation of _m / _2)
        for st, cin, cm, co, dil in ((6, 1024, 512, 512, 2), (5, 1024, 512, 512, 1), (4, 1024, 512, 256, 1),
                                     (3, 512, 256, 128, 1), (2, 256, 128, 64, 1), (1, 128, 64, 64, 1)):
            setattr(self, f"conv{st}d_1", Conv2d(cin, cm, 3, padding=1, bias=True))
            setattr(self, f"bn{st}d_1", BatchNorm2d(cm))
            setattr(self, f"conv{st}d_m", Conv2d(cm, cm, 3, padding=dil, dilation=dil, bias=True))
            setattr(self, f"bn{st}d_m", BatchNorm2d(cm))
            setattr(self, f"conv{st}d_2", Conv2d(cm, co, 3, padding=dil, dilation=dil, bias=True))
            setattr(self, f"bn{st}d_2", BatchNorm2d(co))
        for n, c in (("b", 512), ("6", 512), ("5", 512), ("4", 256), ("3", 128), ("2", 64), ("1", 64)):
            setattr(self, f"outconv{n}", Conv2d(c, 1, 3, padding=1, bias=True))
        self.refunet = RefUnet(1, 64)

    def forward(self, x):
        """-> (sigmoid(dout), sigmoid(d1), sigmoid(d2), ..., sigmoid(d6), sigmoid(db)), each (B,1,H,W) fp32."""
        _check_eval(self, x)
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            raise WsdlError(f"BASNet: H and W must be multiples of 32 (got {H} x {W}): the ceil-mode pools and x2 up-samples "
                            "of the decoder no longer line up (the reference fails in torch.cat)")
        dev = x.device
        x = x.contiguous()
        # decoder stage inputs: torch.cat((up(previous stage) | hbg, skip), 1)
        c = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512, 6: 512}
        bufs = {s: _stage_buffer(B, c[s], H >> (s - 1), W >> (s - 1), dev) for s in (1, 2, 3, 4)}
        bufs[5] = _stage_buffer(B, 512, H >> 4, W >> 4, dev)
        bufs[6] = _stage_buffer(B, 512, H >> 5, W >> 5, dev)

        def skip(s):
            buf, slot = bufs[s]
            return buf[:, c[s]:], slot

        # encoder
        hx = _conv(x, self.inconv, self.inbn, relu=True)
        h = None
        for s, layer in enumerate((self.encoder1, self.encoder2, self.encoder3, self.encoder4), 1):
            out, slot = skip(s)
            h = _run_layer(layer, hx if h is None else h, out=out, y_amax=slot)
        hx = ops.max_pool_2x2_ceil(h)                                    # pool4
        for i, blk in enumerate((self.resb5_1, self.resb5_2, self.resb5_3)):
            hx = blk.run(hx, *(skip(5) if i == 2 else (None, None)))
        h5 = hx
        hx = ops.max_pool_2x2_ceil(h5)                                   # pool5
        for i, blk in enumerate((self.resb6_1, self.resb6_2, self.resb6_3)):
            hx = blk.run(hx, *(skip(6) if i == 2 else (None, None)))
        h6 = hx
        # bridge: hbg straight into the first half of stage 6d's input
        buf6, slot6 = bufs[6]
        hx = _conv(h6, self.convbg_1, self.bnbg_1, relu=True)
        hx = _conv(hx, self.convbg_m, self.bnbg_m, relu=True)
        hbg = _conv(hx, self.convbg_2, self.bnbg_2, relu=True, out=buf6[:, :512], y_amax=slot6)
        # decoder
        hd = {}
        for s in (6, 5, 4, 3, 2, 1):
            buf, _ = bufs[s]
            if s < 6:
                _up_into(hd[s + 1], buf)                                 # upscore2(hd_{s+1})
            hx = _conv(buf, getattr(self, f"conv{s}d_1"), getattr(self, f"bn{s}d_1"), relu=True)
            hx = _conv(hx, getattr(self, f"conv{s}d_m"), getattr(self, f"bn{s}d_m"), relu=True)
            nxt = bufs[s - 1][1] if s > 1 else None                      # hd_s also bounds stage s-1's buffer
            hd[s] = _conv(hx, getattr(self, f"conv{s}d_2"), getattr(self, f"bn{s}d_2"), relu=True, y_amax=nxt)
        # side outputs + refinement: outs[0] = sigmoid(dout), outs[1..6] = sigmoid(d1..d6), outs[7] = sigmoid(db)
        outs = torch.empty(8, B, 1, H, W, device=dev, dtype=torch.float32)
        ops.side_output(hbg, self.outconvb.weight, self.outconvb.bias, 32, out=outs[7])
        for s in (6, 5, 4, 3, 2):
            conv = getattr(self, f"outconv{s}")
            ops.side_output(hd[s], conv.weight, conv.bias, 1 << (s - 1) if s < 6 else 32, out=outs[s])
        _, d1 = ops.side_output(hd[1], self.outconv1.weight, self.outconv1.bias, 1, out=outs[1])
        self.refunet.run(d1, out=outs[0])
        return tuple(outs[i] for i in range(8))
