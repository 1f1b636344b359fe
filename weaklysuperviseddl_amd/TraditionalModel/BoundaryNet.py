"""IRN's class-boundary network (Ahn, Cho & Kwak, "Weakly Supervised Learning of Instance Segmentation with Inter-pixel
Relations", CVPR 2019) on the HIP path.

The reference has no such step; nothing here runs unless it is called.  The network is IRN's edge branch on the frozen ResNet-50
trunk the project already builds (``FrozenResNetCAM``): five bias-free 1 x 1 reductions to 32 channels, one per stage (layer0:
64 channels at stride 4; layer1: 256 at stride 4; layer2: 512 at stride 8; layer3: 1024 and the dilated layer4: 2048 at stride
16), each followed by ReLU, the three coarser maps resized to the stride-4 size, a concatenation to 160 channels and one 1 x 1
convolution with bias to a single map: the boundary LOGITS.  Their sigmoid is the class-boundary map; the affinity of two pixels
is one minus its maximum on the line between them (``ops.path_affinity``).  The logits feed ``ops.path_affinity_loss`` in training
and, through a sigmoid, ``ops.edge_random_walk`` when a CAM is turned into a pseudo mask
(``generate_pseudo_masks(boundary=...)``).  IRN puts GroupNorm(4, 32) behind its reductions: the five stages' activation scales
differ by orders of magnitude, and the normalisation is what lets the head train from a random start.  ``norm="group"`` builds it
(``wnn.GroupNorm`` with the ReLU fused); the default ``norm=None`` is the bare head of before, module for module.  One
difference to IRN remains: the project's order is reduce -> normalise + ReLU -> resize for every stage, where IRN resizes the
three coarser stages BEFORE their ReLU (as ``AffinityNet`` notes its missing ELUs).  IRN's second branch - the displacement
field and the instance centroids - is not built: the data set has one object per image.
"""
import torch
import torch.nn as nn

from .. import nn as wnn
from .. import ops
from .AffinityNet import affinity_labels_from_cam

EDGE_CHANNELS = 32


class BoundaryNet(nn.Module):
    """``BoundaryNet(trunk, norm=None, groups=4)``: ``trunk`` has ``layer0 .. layer4`` (a ``FrozenResNetCAM``); it stays frozen
    and in eval mode.  ``forward(x)`` for images (B,3,H,W) returns the boundary logits (B,1,H/4,W/4).  Trainable: ``fc_edge1 ..
    fc_edge5`` (IRN's names), bias-free 1 x 1 convolutions to 32 channels, and ``fc_edge6``, 160 -> 1 with bias.  ``norm="group"``
    adds ``gn_edge1 .. gn_edge5``, ``wnn.GroupNorm(groups, 32, relu=True)``, behind the five reductions in place of the bare ReLU;
    with ``norm=None`` the network has the same modules, state-dict keys and initial weights as before the option existed."""

    def __init__(self, trunk, norm=None, groups=4):
        super().__init__()
        if norm not in (None, "group"):
            raise ValueError(f"BoundaryNet: norm {norm!r} must be None or 'group'")
        if norm == "group":
            ops.check_group_norm_options(groups, EDGE_CHANNELS, name="BoundaryNet")
        self.norm = norm
        self.trunk = trunk
        for p in self.trunk.parameters():
            p.requires_grad = False
        self.fc_edge1 = wnn.Conv2d(64, EDGE_CHANNELS, 1)
        self.fc_edge2 = wnn.Conv2d(256, EDGE_CHANNELS, 1)
        self.fc_edge3 = wnn.Conv2d(512, EDGE_CHANNELS, 1)
        self.fc_edge4 = wnn.Conv2d(1024, EDGE_CHANNELS, 1)
        self.fc_edge5 = wnn.Conv2d(2048, EDGE_CHANNELS, 1)
        self.fc_edge6 = wnn.Conv2d(5 * EDGE_CHANNELS, 1, 1, bias=True)
        for conv in self._convs():
            nn.init.kaiming_normal_(conv.weight)
        nn.init.zeros_(self.fc_edge6.bias)
        if norm == "group":                     # (ones and zeros: no random draw, the convolutions above are the same either way)
            for i in range(1, 6):
                setattr(self, f"gn_edge{i}", wnn.GroupNorm(groups, EDGE_CHANNELS, relu=True))
        self.trunk.eval()

    def _convs(self):
        return (self.fc_edge1, self.fc_edge2, self.fc_edge3, self.fc_edge4, self.fc_edge5, self.fc_edge6)

    def _norms(self):
        return tuple(getattr(self, f"gn_edge{i}") for i in range(1, 6)) if self.norm == "group" else ()

    def train(self, mode=True):
        super().train(mode)
        self.trunk.eval()                       # frozen: its BatchNorm layers keep their running statistics
        return self

    def head_parameters(self):
        return [p for m in self._convs() + self._norms() for p in m.parameters()]

    def forward(self, x):
        t = self.trunk
        with torch.no_grad():
            f0 = t.layer0(x)
            f1 = t.layer1(f0)
            f2 = t.layer2(f1)
            f3 = t.layer3(f2)
            f4 = t.layer4(f3)
        size = tuple(f1.shape[-2:])
        acts = self._norms() or (ops.relu,) * 5
        maps = [act(conv(f)) for act, conv, f in zip(acts, self._convs(), (f0, f1, f2, f3, f4))]
        maps = [m if tuple(m.shape[-2:]) == size else ops.bilinear_resize(m, size) for m in maps]
        return self.fc_edge6(ops.concat_channels(maps))


def train_boundary_net(model, loader, cams, *, epochs=1, lr=1e-3, lo=0.05, hi=0.3, radius=5, ignore_index=255,
                       weights=ops.AFFINITY_WEIGHTS, optimizer=None, device="cuda", log=print):
    """A short training loop of the head, as ``train_affinity_net``: for every batch ``(imgs, ...)`` of ``loader`` and its CAM -
    ``cams`` is a callable ``cams(imgs) -> (B,H,W)`` in [0, 1] or a sequence with one such tensor per batch - the labels are
    ``affinity_labels_from_cam(cam, lo, hi, logit size)`` and the loss ``wnn.PathAffinityLoss``.  ``optimizer``: one of the
    project's flat optimisers over ``model.head_parameters()`` (default ``FlatAdam(lr=lr)``).  Bad options raise before the model
    is moved to the device.  Returns the per-epoch mean losses (one host read per epoch)."""
    from ..optim import FlatAdam
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"train_boundary_net: epochs {epochs!r} must be an int >= 1")
    if not lo < hi:
        raise ValueError(f"train_boundary_net: lo {lo!r} must be below hi {hi!r}")
    if not callable(cams) and not hasattr(cams, "__getitem__"):
        raise ValueError("train_boundary_net: cams is a callable cams(imgs) -> (B,H,W) or a sequence with one CAM tensor per batch")
    if not isinstance(model, BoundaryNet):
        raise ValueError("train_boundary_net: model must be a BoundaryNet")
    criterion = wnn.PathAffinityLoss(radius, ignore_index, weights)       # (refuses a bad radius / weights before any device work)
    model.to(device).train()
    opt = optimizer if optimizer is not None else FlatAdam(model.head_parameters(), lr=lr)
    history = []
    for epoch in range(epochs):
        total, n = torch.zeros((), device=device), 0
        for j, batch in enumerate(loader):
            imgs = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
            cam = (cams(imgs) if callable(cams) else cams[j]).to(device)
            logits = model(imgs)
            labels = affinity_labels_from_cam(cam, lo, hi, logits.shape[-2:], ignore_index)
            loss = criterion(logits, labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += loss.detach()
            n += 1
        history.append(total.item() / max(n, 1))
        if log:
            log(f"BoundaryNet epoch {epoch + 1}/{epochs} - loss {history[-1]:.5f}")
    model.eval()
    return history
