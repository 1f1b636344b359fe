"""Pixel embeddings for the prototype ops (SIPE: Chen et al., CVPR 2022; pixel-to-prototype contrast: Du et al., CVPR 2022) on
the HIP path.

The reference has no such step; nothing here runs unless it is called.  Two feature sources on the frozen ResNet-50 trunk the
project already builds (``FrozenResNetCAM``): ``TrunkFeatures`` hands out one of the trunk's feature maps as it is - the
training-free path of ``prototype_cam`` - and ``ProjectionNet`` is AffinityNet's head layout (three 1 x 1 reductions of the
stride-8 features of layer2, the stride-16 features of layer3 and the dilated layer4 to 64, 128 and 256 channels, resized to the
stride-8 size and concatenated) followed by one 1 x 1 projection 448 -> ``dim``, trained with ``wnn.PrototypeContrastLoss`` on
seeds taken from the CAM.
"""
import torch
import torch.nn as nn

from .. import nn as wnn
from .. import ops
from .AffinityNet import FEATURE_CHANNELS, affinity_labels_from_cam

_LAYERS = ("layer2", "layer3", "layer4")


class TrunkFeatures(nn.Module):
    """``TrunkFeatures(trunk, layer='layer4')``: ``forward(x)`` for images (B,3,H,W) returns the frozen trunk's features behind
    ``layer`` ('layer2': 512 channels at stride 8, 'layer3': 1024 and 'layer4': 2048 at stride 16), in eval mode and without a
    gradient.  No trainable parameter."""

    def __init__(self, trunk, layer="layer4"):
        super().__init__()
        if layer not in _LAYERS:
            raise ValueError(f"TrunkFeatures: layer {layer!r}: one of {_LAYERS}")
        self.trunk, self.layer = trunk, layer
        for p in self.trunk.parameters():
            p.requires_grad = False
        self.trunk.eval()

    def train(self, mode=True):
        super().train(mode)
        self.trunk.eval()
        return self

    @torch.no_grad()
    def forward(self, x):
        t = self.trunk
        f = t.layer2(t.layer1(t.layer0(x)))
        if self.layer != "layer2":
            f = t.layer3(f)
        if self.layer == "layer4":
            f = t.layer4(f)
        return f


class ProjectionNet(nn.Module):
    """``ProjectionNet(trunk, dim=128)``: ``trunk`` has ``layer0 .. layer4`` (a ``FrozenResNetCAM``); it stays frozen and in eval
    mode.  ``forward(x)`` for images (B,3,H,W) returns the embeddings (B,dim,h,w) at the trunk's stride-8 size (not normalised: the
    prototype ops normalise).  Trainable: ``f8_3``, ``f8_4``, ``f8_5`` (AffinityNet's reductions) and ``proj``, bias-free 1 x 1
    convolutions."""

    def __init__(self, trunk, dim=128):
        super().__init__()
        if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= ops.PROTOTYPE_MAX_CHANNELS:
            raise ValueError(f"ProjectionNet: dim {dim!r} must be an int in [1, {ops.PROTOTYPE_MAX_CHANNELS}]")
        self.trunk, self.dim = trunk, dim
        for p in self.trunk.parameters():
            p.requires_grad = False
        self.f8_3 = wnn.Conv2d(512, 64, 1)
        self.f8_4 = wnn.Conv2d(1024, 128, 1)
        self.f8_5 = wnn.Conv2d(2048, 256, 1)
        self.proj = wnn.Conv2d(FEATURE_CHANNELS, dim, 1)
        for conv in (self.f8_3, self.f8_4, self.f8_5, self.proj):
            nn.init.kaiming_normal_(conv.weight)
        self.trunk.eval()

    def train(self, mode=True):
        super().train(mode)
        self.trunk.eval()                       # frozen: its BatchNorm layers keep their running statistics
        return self

    def head_parameters(self):
        return [p for conv in (self.f8_3, self.f8_4, self.f8_5, self.proj) for p in conv.parameters()]

    def forward(self, x):
        t = self.trunk
        with torch.no_grad():
            f2 = t.layer2(t.layer1(t.layer0(x)))
            f3 = t.layer3(f2)
            f4 = t.layer4(f3)
        size = tuple(f2.shape[-2:])
        a = ops.relu(self.f8_3(f2))
        b = ops.relu(self.f8_4(f3))
        c = ops.relu(self.f8_5(f4))
        if tuple(b.shape[-2:]) != size:
            b, c = ops.bilinear_resize(b, size), ops.bilinear_resize(c, size)
        return self.proj(ops.concat_channels([a, b, c]))


def train_projection_net(model, loader, cams, *, epochs=1, lr=1e-3, lo=0.05, hi=0.3, temperature=0.1, source="batch", momentum=0.99,
                         ignore_index=255, optimizer=None, device="cuda", log=print):
    """A short training loop of the head, ``train_affinity_net``'s: for every batch ``(imgs, ...)`` of ``loader`` and its CAM -
    ``cams`` is a callable ``cams(imgs) -> (B,H,W)`` in [0, 1] or a sequence with one such tensor per batch - the labels are
    ``affinity_labels_from_cam(cam, lo, hi, feature size)`` (0 sure background, 1 sure foreground) and the loss
    ``wnn.PrototypeContrastLoss(2, temperature, source, momentum)``.  ``optimizer``: one of the project's flat optimisers over
    ``model.head_parameters()`` (default ``FlatAdam(lr=lr)``).  Bad options raise before the model is moved to the device.
    Returns the per-epoch mean losses (one host read per epoch)."""
    from ..optim import FlatAdam
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"train_projection_net: epochs {epochs!r} must be an int >= 1")
    if not lo < hi:
        raise ValueError(f"train_projection_net: lo {lo!r} must be below hi {hi!r}")
    if not callable(cams) and not hasattr(cams, "__getitem__"):
        raise ValueError("train_projection_net: cams is a callable cams(imgs) -> (B,H,W) or a sequence with one CAM tensor per batch")
    if not hasattr(model, "head_parameters"):
        raise ValueError("train_projection_net: model must be a ProjectionNet")
    criterion = wnn.PrototypeContrastLoss(2, temperature, source, momentum, ignore_index)      # (refuses bad options before any device work)
    model.to(device).train()
    opt = optimizer if optimizer is not None else FlatAdam(model.head_parameters(), lr=lr)
    history = []
    for epoch in range(epochs):
        total, n = torch.zeros((), device=device), 0
        for j, batch in enumerate(loader):
            imgs = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
            cam = (cams(imgs) if callable(cams) else cams[j]).to(device)
            feat = model(imgs)
            labels = affinity_labels_from_cam(cam, lo, hi, feat.shape[-2:], ignore_index)
            loss = criterion(feat, labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += loss.detach()
            n += 1
        history.append(total.item() / max(n, 1))
        if log:
            log(f"ProjectionNet epoch {epoch + 1}/{epochs} - loss {history[-1]:.5f}")
    model.eval()
    return history
