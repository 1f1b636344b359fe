"""AffinityNet (Ahn & Kwak, "Learning Pixel-level Semantic Affinity with Image-level Supervision", CVPR 2018) on the HIP path.

The reference has no such step; nothing here runs unless it is called.  The network is PSA's head on the frozen ResNet-50
trunk the project already builds (``FrozenResNetCAM``: stride-8 features from layer2, stride-16 features from layer3 and the
dilated layer4): three 1 x 1 reductions (64, 128 and 256 channels), the stride-16 maps resized to the stride-8 size, a
concatenation and one 1 x 1 convolution 448 -> 448.  Its output feeds ``ops.affinity_loss`` in training and
``ops.affinity_random_walk`` when a CAM is turned into a pseudo mask (``generate_pseudo_masks(affinity=...)``).  PSA puts ELUs
behind its convolutions; the library's activation is ReLU, used behind the three reductions (the last convolution is linear:
the features are compared by their L1 distance).
"""
import torch
import torch.nn as nn

from .. import nn as wnn
from .. import ops
from .PsuedoMasks import nearest_resize_index, seeds_from_cam

FEATURE_CHANNELS = 448


class AffinityNet(nn.Module):
    """``AffinityNet(trunk)``: ``trunk`` has ``layer0 .. layer4`` (a ``FrozenResNetCAM``); it stays frozen and in eval mode.
    ``forward(x)`` for images (B,3,H,W) returns the features (B,448,h,w) at the trunk's stride-8 size.  Trainable: ``f8_3``,
    ``f8_4``, ``f8_5`` and ``f9`` (PSA's names), bias-free 1 x 1 convolutions."""

    def __init__(self, trunk):
        super().__init__()
        self.trunk = trunk
        for p in self.trunk.parameters():
            p.requires_grad = False
        self.f8_3 = wnn.Conv2d(512, 64, 1)
        self.f8_4 = wnn.Conv2d(1024, 128, 1)
        self.f8_5 = wnn.Conv2d(2048, 256, 1)
        self.f9 = wnn.Conv2d(FEATURE_CHANNELS, FEATURE_CHANNELS, 1)
        for conv in (self.f8_3, self.f8_4, self.f8_5, self.f9):
            nn.init.kaiming_normal_(conv.weight)
        self.trunk.eval()

    def train(self, mode=True):
        super().train(mode)
        self.trunk.eval()                       # frozen: its BatchNorm layers keep their running statistics
        return self

    def head_parameters(self):
        return [p for conv in (self.f8_3, self.f8_4, self.f8_5, self.f9) for p in conv.parameters()]

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
        return self.f9(ops.concat_channels([a, b, c]))


def affinity_labels_from_cam(cam, lo, hi, size, ignore_index=255):
    """Training labels for ``ops.affinity_loss`` from a CAM (B,H,W) in [0, 1]: ``seeds_from_cam`` (1 where ``cam >= hi``, 0 where
    ``cam <= lo``, ``ignore_index`` between) followed by a nearest-neighbour down-sample to ``size`` = (h, w), the feature
    size.  int64 (B,h,w) on the CAM's device."""
    seeds = seeds_from_cam(cam, lo, hi, ignore_index)
    if seeds.dim() != 3:
        raise ValueError(f"affinity_labels_from_cam: cam {tuple(seeds.shape)} must be (B,H,W)")
    h, w = int(size[0]), int(size[1])
    iy = nearest_resize_index(h, seeds.shape[1], seeds.device)
    ix = nearest_resize_index(w, seeds.shape[2], seeds.device)
    return seeds[:, iy][:, :, ix].contiguous()


def train_affinity_net(model, loader, cams, *, epochs=1, lr=1e-3, lo=0.05, hi=0.3, radius=5, ignore_index=255,
                       weights=ops.AFFINITY_WEIGHTS, optimizer=None, device="cuda", log=print):
    """A short training loop of the head: for every batch ``(imgs, ...)`` of ``loader`` and its CAM - ``cams`` is a callable
    ``cams(imgs) -> (B,H,W)`` in [0, 1] or a sequence with one such tensor per batch - the labels are
    ``affinity_labels_from_cam(cam, lo, hi, feature size)`` and the loss ``wnn.AffinityLoss``.  ``optimizer``: one of the
    project's flat optimisers over ``model.head_parameters()`` (default ``FlatAdam(lr=lr)``).  Bad options raise before the model
    is moved to the device.  Returns the per-epoch mean losses
    (one host read per epoch)."""
    from ..optim import FlatAdam
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"train_affinity_net: epochs {epochs!r} must be an int >= 1")
    if not lo < hi:
        raise ValueError(f"train_affinity_net: lo {lo!r} must be below hi {hi!r}")
    if not callable(cams) and not hasattr(cams, "__getitem__"):
        raise ValueError("train_affinity_net: cams is a callable cams(imgs) -> (B,H,W) or a sequence with one CAM tensor per batch")
    if not hasattr(model, "head_parameters"):
        raise ValueError("train_affinity_net: model must be an AffinityNet")
    criterion = wnn.AffinityLoss(radius, ignore_index, weights)           # (refuses a bad radius / weights before any device work)
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
            log(f"AffinityNet epoch {epoch + 1}/{epochs} - loss {history[-1]:.5f}")
    model.eval()
    return history
