"""Parameter-holding modules for the HIP path.

They keep torchvision's attribute / state_dict names (conv1.weight, bn1.running_mean, downsample.0.weight,
classifier.0.convs.1.0.weight ...) so real weights drop in, but never call an ATen compute op: every
forward goes through ``ops`` (libwsdl_hip.so).  ``FusedSequential`` runs Conv2d -> BatchNorm2d [-> ReLU]
triples as one fused node (conv + BN statistics/apply + activation).
"""
import math

import torch
import torch.nn as nn

from . import ops


class Conv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0, dilation=1, bias=False):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.empty(cout)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # nn.Conv2d default init (kaiming_uniform a=sqrt(5)); model builders re-init as torchvision does
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size * self.kernel_size)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return ops.conv_bias_act(x, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                 cache=self.__dict__.setdefault("_wsdl_cache", {}))

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, k={self.kernel_size}, s={self.stride}, "
                f"p={self.padding}, d={self.dilation}, bias={self.bias is not None}")


class BatchNorm2d(nn.Module):
    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self._pending_steps = 0     # train-mode forwards not yet folded into num_batches_tracked

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        if self._pending_steps:
            self.num_batches_tracked += self._pending_steps
            self._pending_steps = 0
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kwargs):
        self._pending_steps = 0
        super()._load_from_state_dict(*args, **kwargs)

    def forward(self, x):
        # the models run BatchNorm fused behind the convolution (FusedSequential / conv_bn); a stand-alone call - a
        # drop-in user doing model.backbone.bn1(x) - takes the same kernels without the convolution
        if self.training:
            self._pending_steps += 1
        return ops.batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, self.momentum, self.eps,
                              self.training)


class GroupNorm(nn.Module):
    """``torch.nn.GroupNorm`` on the HIP path (``ops.group_norm``): torch's parameter names and initial values (``weight`` ones,
    ``bias`` zeros), so its state dict loads; no buffers, train and eval are the same function.  ``relu=True`` fuses the
    activation into the same launches.  Unlike torch's, a group of one element is accepted."""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True, relu=False):
        super().__init__()
        ops.check_group_norm_options(num_groups, num_channels, eps, name="GroupNorm")
        self.num_groups, self.num_channels, self.eps, self.affine, self.relu = num_groups, num_channels, eps, bool(affine), bool(relu)
        if self.affine:
            self.weight = nn.Parameter(torch.ones(num_channels))
            self.bias = nn.Parameter(torch.zeros(num_channels))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def forward(self, x):
        if x.dim() < 2 or x.shape[1] != self.num_channels:
            raise ops.WsdlError(f"GroupNorm: expected (B, {self.num_channels}, *), got {tuple(x.shape)}")
        return ops.group_norm(x, self.num_groups, self.weight, self.bias, self.eps, self.relu)

    def extra_repr(self):
        return f"{self.num_groups}, {self.num_channels}, eps={self.eps}, affine={self.affine}, relu={self.relu}"


class ReLU(nn.Module):
    def forward(self, x):
        # fused into the producing kernel inside the models; stand-alone (hooked / called directly) it is one launch
        return ops.relu(x)


class MaxPool3x3s2(nn.Module):
    def forward(self, x):
        return ops.max_pool_3x3_s2(x)


class GlobalAvgPool(nn.Module):
    """nn.AdaptiveAvgPool2d(1)"""

    def forward(self, x):
        return ops.global_avg_pool(x)


class Dropout(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p
        self.injected_mask = None   # parity tests: uint8 mask used instead of the device RNG
        self._seed = None           # host seed, drawn once; the per-call variation is a device counter (graph-safe)
        self._counter = None

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        if self.injected_mask is not None:
            return ops.dropout(x, self.p, True, mask=self.injected_mask)
        if self._seed is None or self._counter is None or self._counter.device != x.device:
            self._seed = (int(torch.randint(0, 2 ** 62, (1,)).item()) + ops.DROPOUT_SEED_OFFSET[0]) % (1 << 62)
            self._counter = torch.zeros(1, dtype=torch.int64, device=x.device)
        return ops.dropout(x, self.p, True, seed=self._seed, counter=self._counter)


class Linear(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        self.in_features, self.out_features = fin, fout
        self.weight = nn.Parameter(torch.empty(fout, fin))
        self.bias = nn.Parameter(torch.empty(fout))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.uniform_(self.bias, -1.0 / math.sqrt(fin), 1.0 / math.sqrt(fin))

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias)


def conv_bn(x, conv, bn, relu, residual=None, passthrough=False, link=None, out_holder=None):
    """conv -> bn (batch stats when bn.training, folded running stats otherwise) -> +residual -> relu."""
    if conv.bias is not None:
        raise RuntimeError("conv_bn: a conv followed by BN carries no bias on this path")
    if bn.training:
        bn._pending_steps += 1      # momentum is fixed, so the counter never feeds the arithmetic
    cache = conv.__dict__.setdefault("_wsdl_cache", {})         # derived tensors, keyed on versions / epochs
    return ops.conv_bn_act(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.stride,
                           conv.padding, conv.dilation, relu, residual, bn.momentum, bn.eps, bn.training, cache,
                           passthrough, link, out_holder if bn.training else None)


class FusedSequential(nn.Sequential):
    """nn.Sequential whose Conv2d, BatchNorm2d[, ReLU] runs execute as single fused nodes."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, Conv2d) and i + 1 < len(mods) and isinstance(mods[i + 1], BatchNorm2d):
                relu = i + 2 < len(mods) and isinstance(mods[i + 2], ReLU)
                x = conv_bn(x, m, mods[i + 1], relu)
                i += 3 if relu else 2
            else:
                x = m(x)
                i += 1
        return x


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride=stride, padding=dilation, dilation=dilation)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = ReLU()
        self.downsample = downsample

    def forward(self, x):
        # x feeds conv1 AND the identity / downsample branch: route the second use through conv1's node (see
        # ops.conv_bn_act) so that the two input gradients are summed in conv1's dgrad epilogue
        # identity blocks in train mode: the identity branch's gradient goes from the last node to the first through an
        # ops.IdentityLink instead of through a tensor of its own
        train = self.bn1.training and self.bn3.training and torch.is_grad_enabled()
        ds = self.downsample
        proj = (train and ds is not None and len(ds) == 2 and isinstance(ds[0], Conv2d) and isinstance(ds[1], BatchNorm2d)
                and ds[1].training and ds[0].bias is None)
        link = ops.IdentityLink(projection=proj) if (train and (ds is None or proj)) else None
        y, idt = conv_bn(x, self.conv1, self.bn1, True, passthrough=True, link=None if proj else link)
        if proj:
            idt = conv_bn(idt, ds[0], ds[1], False, link=link)       # the projection shortcut, joined to the last node
        elif ds is not None:
            idt = ds(idt)
        y = conv_bn(y, self.conv2, self.bn2, True)
        return conv_bn(y, self.conv3, self.bn3, True, residual=idt, link=link)   # relu(bn3(conv3) + identity)


def make_resnet50_stages(replace_stride_with_dilation):
    """-> (conv1, bn1, layer1..layer4) with torchvision ResNet-50 v1.5 wiring and initialisation."""
    state = {"inplanes": 64, "dilation": 1}

    def stage(planes, blocks, stride, dilate):
        prev = state["dilation"]
        if dilate:
            state["dilation"] *= stride
            stride = 1
        down = None
        if stride != 1 or state["inplanes"] != planes * 4:
            down = FusedSequential(Conv2d(state["inplanes"], planes * 4, 1, stride=stride), BatchNorm2d(planes * 4))
        mods = [Bottleneck(state["inplanes"], planes, stride, prev, down)]
        state["inplanes"] = planes * 4
        for _ in range(1, blocks):
            mods.append(Bottleneck(state["inplanes"], planes, 1, state["dilation"], None))
        return nn.Sequential(*mods)

    conv1 = Conv2d(3, 64, 7, stride=2, padding=3)
    bn1 = BatchNorm2d(64)
    r = replace_stride_with_dilation
    layers = [stage(64, 3, 1, False), stage(128, 4, 2, r[0]), stage(256, 6, 2, r[1]), stage(512, 3, 2, r[2])]
    for m in [conv1] + [mm for l in layers for mm in l.modules()]:
        if isinstance(m, Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return conv1, bn1, layers


class _Criterion(nn.Module):
    """What the loss criteria below share, so that a launch plan (``plan.host_scalars``) sees them alike.  Every option is a
    plain attribute and so part of the plan key: changing one records a new plan instead of replaying a stale one; a value that
    is to change WITHOUT a new plan lives in a one-element device buffer.  Buffers the object fills are allocated anew only
    when the shape changes, so their addresses - which a plan freezes - stay put; the address of every buffer named in
    ``_pointers`` is kept in the attribute ``<name>_ptr`` (0 while there is none) and the shape of every one in ``_shapes`` in
    the string ``<name>_shape`` ("" while there is none), refreshed by ``_refresh_pointers`` - after ``.to(device)``, after a
    call that may have replaced a buffer (``_adopt``) and before the loss is taken."""

    _pointers = ()
    _shapes = ()

    def _class_weight(self, weight):
        """``weight`` (None or a (C,) tensor) as this object's own float32 copy."""
        if weight is not None and (not torch.is_tensor(weight) or weight.dim() != 1):
            raise ValueError(f"{type(self).__name__}: weight must be a (C,) tensor")
        return None if weight is None else weight.detach().to(torch.float32).clone()

    def _refresh_pointers(self):
        for name in self._pointers:
            t = getattr(self, name)
            setattr(self, name + "_ptr", 0 if t is None else t.data_ptr())
        for name in self._shapes:
            t = getattr(self, name)
            setattr(self, name + "_shape", "" if t is None else "x".join(str(d) for d in t.shape))

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)      # .to(device) / .cuda() move the buffers
        self._refresh_pointers()
        return out

    def _adopt(self, bufs, names):
        """After an ``out=bufs`` call of ``ops``: the tensors it created become this object's buffers (``names``: key -> buffer)."""
        for k, name in names.items():
            if getattr(self, name) is not bufs[k]:
                setattr(self, name, bufs[k])
        self._refresh_pointers()

    def _set_pixel_weight(self, t):
        """Copy a float32 (B,H,W) map into the ``pixel_weight`` buffer (allocated anew only when the shape changes); None drops it."""
        if t is None:
            self.pixel_weight = None
        else:
            if not torch.is_tensor(t) or t.dim() != 3:
                raise ValueError(f"{type(self).__name__}.set_pixel_weight: a (B,H,W) tensor or None")
            cur = self.pixel_weight
            if cur is None or cur.shape != t.shape or cur.device != t.device:
                self.pixel_weight = torch.empty(t.shape, device=t.device, dtype=torch.float32)
            self.pixel_weight.copy_(t.detach())
        self._refresh_pointers()
        return self


class CrossEntropyLoss(_Criterion):
    """``torch.nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing)`` on (B,C,H,W) logits and (B,H,W)
    labels, run by the fused cross-entropy kernel (``ops.cross_entropy``), plus a per-pixel confidence weight that lives
    on the device.

    ``set_pixel_weight(t)`` copies a float32 (B,H,W) map (finite, >= 0; 0 = ignore the pixel) into a buffer this object
    owns; the buffer is allocated anew only when the shape changes, so its address - which a launch plan freezes - stays
    put while the values change every step.  ``set_pixel_weight(None)`` drops it.  The smoothing factor, the reduction,
    ``ignore_index``, the addresses of both buffers and the shape of the pixel weights are plain attributes: ``plan.host_scalars`` puts them into the
    plan key, so changing one records a new plan instead of replaying a stale one.

    Pseudo masks with a confidence, e.g. from the CRF posterior or from the CAM's distance to its threshold::

        crit = wnn.CrossEntropyLoss(weight=ops.class_weights_from_labels(masks, 2), label_smoothing=0.1)
        refined, q = ops.dense_crf(images_u8, unary, return_q=True)       # q: (B,2,H,W) posterior
        crit.set_pixel_weight(q.amax(1))                                    # or (2 * cam - 1).abs() for a CAM in [0, 1]
        loss = train_step(model, optimizer, images, refined, criterion=crit)
    """

    _pointers = ("weight", "pixel_weight")
    _shapes = ("pixel_weight",)

    def __init__(self, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
        super().__init__()
        ops.check_cross_entropy_options(reduction, label_smoothing)
        self.register_buffer("weight", self._class_weight(weight))
        self.register_buffer("pixel_weight", None, persistent=False)
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self._refresh_pointers()

    set_pixel_weight = _Criterion._set_pixel_weight

    def forward(self, logits, labels):
        self._refresh_pointers()
        return ops.cross_entropy(logits, labels.long(), self.ignore_index, weight=self.weight,
                                 label_smoothing=self.label_smoothing, reduction=self.reduction,
                                 pixel_weight=self.pixel_weight)

    def extra_repr(self):
        return (f"ignore_index={self.ignore_index}, reduction={self.reduction!r}, label_smoothing={self.label_smoothing}, "
                f"weight={self.weight is not None}, pixel_weight={None if self.pixel_weight is None else tuple(self.pixel_weight.shape)}")


class MinedCrossEntropyLoss(_Criterion):
    """Cross entropy over the pixels their own loss selects (``ops.cross_entropy_mined``): ``mode="hard"`` is online hard
    example mining / bootstrapped cross entropy - the pixels whose true-class probability is at most ``thresh``, at least
    ``min_kept`` per image - and ``mode="trim"`` drops the fraction ``drop_frac`` of largest loss, the guard against the
    label noise of pseudo masks.  ``scope="batch"`` ranks the pixels of the whole batch (``min_kept * B`` of them),
    ``"image"`` each image by itself.  The selection is made on the device from a count that never reaches the host, ties
    at the threshold are all kept (see ``ops.cross_entropy_mined``), and ``weight`` / ``label_smoothing`` / ``reduction``
    ('mean' or 'sum') apply to the kept pixels as in ``CrossEntropyLoss``.

    Conventions of ``CrossEntropyLoss``: ``set_pixel_weight(t)`` copies a (B,H,W) confidence map into a buffer this object
    owns (a pixel of weight 0 is no candidate); ``threshold`` (float32), ``kept`` and ``valid`` (int64, one entry per scope
    segment) and ``selection`` (float32 (B,H,W): the weights the loss was taken with) are buffers of this object, filled by
    every call and allocated anew only when the shape changes, so the addresses a launch plan freezes stay put; every option
    and every address is a plain attribute, so ``plan.host_scalars`` puts them into the plan key and a changed ``drop_frac``
    records a new plan.  Read the statistics after the step; reading them synchronises, the step does not.  (The one step that
    records a launch plan verifies it on a probe batch and leaves the probe's statistics in the buffers.)

    Under data parallelism each rank selects within its own shard: ``scope="batch"`` means the rank's batch, and the ranks'
    thresholds differ.

        crit = wnn.MinedCrossEntropyLoss(mode="trim", drop_frac=0.2, scope="image")     # noisy pseudo masks
        loss = train_step(model, optimizer, images, pseudo_masks, criterion=crit)
    """

    _pointers = ("weight", "pixel_weight", "threshold", "kept", "valid", "selection")
    _shapes = ("pixel_weight",)

    def __init__(self, mode="hard", thresh=0.7, min_kept=0, drop_frac=0.0, scope="batch", weight=None, ignore_index=-100,
                 reduction="mean", label_smoothing=0.0):
        super().__init__()
        ops.check_mining_options(mode, thresh, min_kept, drop_frac, scope, reduction, label_smoothing)
        self.register_buffer("weight", self._class_weight(weight))
        for name in ("pixel_weight", "threshold", "kept", "valid", "selection"):
            self.register_buffer(name, None, persistent=False)
        self.mode = mode
        self.thresh = None if thresh is None else float(thresh)
        self.min_kept = int(min_kept)
        self.drop_frac = float(drop_frac)
        self.scope = scope
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self._refresh_pointers()

    set_pixel_weight = _Criterion._set_pixel_weight

    def forward(self, logits, labels):
        # (options may have been assigned since the constructor checked them)
        ops.check_mining_options(self.mode, self.thresh, self.min_kept, self.drop_frac, self.scope, self.reduction,
                                 self.label_smoothing)
        stats = {k: getattr(self, k) for k in ("threshold", "kept", "valid", "selection")}
        loss = ops.cross_entropy_mined(logits, labels.long(), self.ignore_index, mode=self.mode, thresh=self.thresh,
                                       min_kept=self.min_kept, drop_frac=self.drop_frac, scope=self.scope, weight=self.weight,
                                       label_smoothing=self.label_smoothing, pixel_weight=self.pixel_weight,
                                       reduction=self.reduction, stats=stats)
        self._adopt(stats, {k: k for k in stats})
        return loss

    def extra_repr(self):
        return (f"mode={self.mode!r}, thresh={self.thresh}, min_kept={self.min_kept}, drop_frac={self.drop_frac}, "
                f"scope={self.scope!r}, ignore_index={self.ignore_index}, reduction={self.reduction!r}, "
                f"label_smoothing={self.label_smoothing}, weight={self.weight is not None}")


class BoundaryAwareCrossEntropyLoss(_Criterion):
    """Cross entropy that trusts a label map less near its own boundary - where the label noise of a CAM-derived pseudo
    mask sits: every call computes ``ops.boundary_confidence(labels, sigma, floor, value)`` - ``floor + (1 - floor) (1 -
    exp(-d^2 / (2 sigma^2)))`` with ``d`` the Euclidean distance of a pixel to the contour of ``labels == value``, 1 in an
    image without a contour - into its own ``pixel_weight`` buffer and hands it to the fused cross entropy
    (``ops.cross_entropy(..., pixel_weight=)``).  ``floor=1`` is the plain cross entropy with a weight of ones.
    ``weight`` / ``ignore_index`` / ``reduction`` / ``label_smoothing`` as in ``CrossEntropyLoss``; 'mean' divides by the
    sum of the weights, so the loss keeps its scale.

    Conventions of ``CrossEntropyLoss``: ``pixel_weight`` (float32) and the two distance planes ``d2_out`` / ``d2_in``
    (int32; ``ops.edt``) are buffers of this object, filled by every call and allocated anew only when the shape changes,
    so the addresses a launch plan freezes stay put; every option and every address is a plain attribute, so
    ``plan.host_scalars`` puts them into the plan key and a changed ``sigma`` records a new plan.  Everything is a launch
    of the library without a host read: ``train_step`` replays one launch plan.

        crit = wnn.BoundaryAwareCrossEntropyLoss(sigma=3.0, floor=0.2)
        loss = train_step(model, optimizer, images, pseudo_masks, criterion=crit)
    """

    _pointers = ("weight", "pixel_weight", "d2_out", "d2_in")
    _shapes = ("pixel_weight",)

    def __init__(self, sigma=3.0, floor=0.0, value=1, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
        super().__init__()
        ops.check_cross_entropy_options(reduction, label_smoothing)
        ops.check_boundary_confidence_options(sigma, floor)
        self.register_buffer("weight", self._class_weight(weight))
        for name in ("pixel_weight", "d2_out", "d2_in"):
            self.register_buffer(name, None, persistent=False)
        self.sigma = float(sigma)
        self.floor = float(floor)
        self.value = int(value)
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self._refresh_pointers()

    def forward(self, logits, labels):
        # (options may have been assigned since the constructor checked them)
        ops.check_cross_entropy_options(self.reduction, self.label_smoothing)
        labels = labels.long()
        bufs = {"weight": self.pixel_weight, "out": self.d2_out, "in": self.d2_in}
        ops.boundary_confidence(labels, self.sigma, self.floor, self.value, out=bufs)
        self._adopt(bufs, {"weight": "pixel_weight", "out": "d2_out", "in": "d2_in"})
        return ops.cross_entropy(logits, labels, self.ignore_index, weight=self.weight, label_smoothing=self.label_smoothing,
                                 reduction=self.reduction, pixel_weight=self.pixel_weight)

    def extra_repr(self):
        return (f"sigma={self.sigma}, floor={self.floor}, value={self.value}, ignore_index={self.ignore_index}, "
                f"reduction={self.reduction!r}, label_smoothing={self.label_smoothing}, weight={self.weight is not None}")


class BoundaryLoss(_Criterion):
    """The boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced segmentation", MIDL 2019):
    ``mean(softmax(logits)_c * phi_c)`` over the valid pixels and the listed ``classes``, ``phi_c`` the signed distance map of
    class ``c`` in ``labels`` (``ops.signed_distance_classes``: negative inside the class, positive outside, 0 for an image
    the class is absent from or fills).  Every call fills its own ``phi`` buffer from ``labels`` and runs the fused kernel
    (``ops.boundary_loss``); pixels with ``labels == ignore_index`` do not count.  It is an additive regulariser - see
    ``CrossEntropyBoundaryLoss``; on its own it is unbounded below.

    Conventions of ``BoundaryAwareCrossEntropyLoss``: ``phi`` (float32 (B,K,H,W)) and the two distance planes ``d2_out`` /
    ``d2_in`` (int32) are buffers of this object, allocated anew only when the shape changes, so the addresses a launch
    plan freezes stay put; the options (``classes`` as the string ``classes_key``) and every address are plain attributes,
    so ``plan.host_scalars`` puts them into the plan key and changed ``classes`` record a new plan.  ``scale_dev``: an
    optional one-element float32 device tensor that multiplies the loss (``ops.boundary_loss(scale=)``)."""

    _pointers = ("phi", "d2_out", "d2_in", "scale_dev")
    _shapes = ("phi",)

    def __init__(self, classes=(1,), ignore_index=-100):
        super().__init__()
        for name in ("phi", "d2_out", "d2_in", "scale_dev"):
            self.register_buffer(name, None, persistent=False)
        self.set_classes(classes)
        self.ignore_index = int(ignore_index)
        self._refresh_pointers()

    def set_classes(self, classes):
        self.classes = ops.check_boundary_classes(classes, type(self).__name__)
        self.classes_key = ",".join(str(c) for c in self.classes)
        return self

    def forward(self, logits, labels):
        # (classes may have been assigned since the constructor checked them)
        self.set_classes(self.classes)
        labels = labels.long()
        bufs = {"phi": self.phi, "out": self.d2_out, "in": self.d2_in}
        ops.signed_distance_classes(labels, self.classes, out=bufs)
        self._adopt(bufs, {"phi": "phi", "out": "d2_out", "in": "d2_in"})
        return ops.boundary_loss(logits, self.phi, labels, classes=self.classes, ignore_index=self.ignore_index,
                                 scale=self.scale_dev)

    def extra_repr(self):
        return f"classes={self.classes}, ignore_index={self.ignore_index}"


class CrossEntropyBoundaryLoss(_Criterion):
    """``cross entropy + alpha * boundary loss`` (Kervadec et al., MIDL 2019, combine a regional loss with the boundary term):
    ``ops.cross_entropy(logits, labels, weight=, ignore_index=, label_smoothing=)`` plus ``BoundaryLoss(classes,
    ignore_index)`` scaled by ``alpha``, added by the library's kernels (``ops.fanout`` / ``ops.add_scalars``), so
    ``train_step`` replays one launch plan.

    ``alpha`` lives in the one-element device buffer ``alpha_dev`` and is read by the kernel: the paper raises it every
    epoch, and ``set_alpha(a)`` writes the buffer WITHOUT a new plan (a host float would be part of the plan key -
    ``plan.host_scalars``).  ``alpha = 0`` is the cross entropy bit for bit.  The signed distance maps are rebuilt from
    ``labels`` on every call (``boundary.phi``).

        crit = wnn.CrossEntropyBoundaryLoss(alpha=0.01, classes=(1,)).to(device)
        for epoch in range(epochs):
            crit.set_alpha(min(1.0, 0.01 * (epoch + 1)))
            loss = train_step(model, optimizer, images, masks, criterion=crit)
    """

    _pointers = ("weight", "alpha_dev")

    def __init__(self, alpha=0.01, classes=(1,), weight=None, ignore_index=-100, label_smoothing=0.0):
        super().__init__()
        ops.check_cross_entropy_options("mean", label_smoothing)
        alpha = self._check_alpha(alpha)
        self.register_buffer("weight", self._class_weight(weight))
        self.register_buffer("alpha_dev", torch.tensor([alpha], dtype=torch.float32), persistent=False)
        self.boundary = BoundaryLoss(classes, ignore_index)
        self.ignore_index = int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        self._refresh_pointers()

    @staticmethod
    def _check_alpha(alpha):
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha < float("inf"):
            raise ValueError(f"CrossEntropyBoundaryLoss: alpha {alpha!r} must be a finite number >= 0")
        return float(alpha)

    def set_alpha(self, alpha):
        """Write ``alpha`` into the device buffer (a stream-ordered fill; the buffer keeps its address)."""
        self.alpha_dev.fill_(self._check_alpha(alpha))
        return self

    def forward(self, logits, labels):
        ops.check_cross_entropy_options("mean", self.label_smoothing)
        self._refresh_pointers()
        labels = labels.long()
        self.boundary.ignore_index = self.ignore_index
        self.boundary.scale_dev = self.alpha_dev
        a, b = ops.fanout(logits, 2)
        ce = ops.cross_entropy(a, labels, self.ignore_index, weight=self.weight, label_smoothing=self.label_smoothing)
        return ops.add_scalars(ce, self.boundary(b, labels))

    def extra_repr(self):
        return (f"classes={self.boundary.classes}, ignore_index={self.ignore_index}, label_smoothing={self.label_smoothing}, "
                f"weight={self.weight is not None}")


class TverskyLoss(_Criterion):
    """The Tversky loss (Salehi et al., MLMI 2017) of ``ops.tversky_loss``: the mean over segments (the images with
    ``per_image``, else the batch) and listed ``classes`` (None: all) of ``(1 - T) ** gamma``, ``T = (I + smooth) / (I + alpha
    FP + beta FN + smooth)`` from the soft intersection, false positives and false negatives of ``softmax(logits)`` against
    ``labels``.  ``alpha = beta = 0.5`` is soft Dice (``DiceLoss``); ``gamma = 1 / gamma_paper`` is the focal Tversky loss of
    Abraham & Khan (ISBI 2019).  ``present_only`` leaves out the classes a segment has no pixel of.

    Conventions of ``BoundaryLoss``: the options (``classes`` as the string ``classes_key``) are plain attributes, so
    ``plan.host_scalars`` puts them into the plan key and a changed ``alpha`` records a new plan.  ``scale_dev``: an optional
    one-element float32 device tensor that multiplies the loss (``ops.tversky_loss(scale=)``) and may change under a plan.

        loss = train_step(model, optimizer, images, masks, criterion=wnn.TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75))
    """

    _pointers = ("scale_dev",)

    def __init__(self, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False,
                 ignore_index=-100):
        super().__init__()
        self._check(alpha, beta, gamma, smooth)
        self.register_buffer("scale_dev", None, persistent=False)
        self.alpha, self.beta, self.gamma, self.smooth = float(alpha), float(beta), float(gamma), float(smooth)
        self.set_classes(classes)
        self.per_image = bool(per_image)
        self.present_only = bool(present_only)
        self.ignore_index = int(ignore_index)
        self._refresh_pointers()

    def _check(self, alpha, beta, gamma, smooth):
        ops.check_tversky_options(alpha, beta, gamma, smooth, type(self).__name__)

    def set_classes(self, classes):
        self.classes = ops.check_overlap_classes(classes, None, type(self).__name__)
        self.classes_key = "all" if self.classes is None else ",".join(str(c) for c in self.classes)
        return self

    def forward(self, logits, labels):
        # (options may have been assigned since the constructor checked them)
        self._check(self.alpha, self.beta, self.gamma, self.smooth)
        self.set_classes(self.classes)
        self._refresh_pointers()
        return ops.tversky_loss(logits, labels.long(), alpha=self.alpha, beta=self.beta, gamma=self.gamma, smooth=self.smooth,
                                classes=self.classes, per_image=self.per_image, present_only=self.present_only,
                                ignore_index=self.ignore_index, scale=self.scale_dev)

    def extra_repr(self):
        return (f"alpha={self.alpha}, beta={self.beta}, gamma={self.gamma}, smooth={self.smooth}, classes={self.classes}, "
                f"per_image={self.per_image}, present_only={self.present_only}, ignore_index={self.ignore_index}")


class DiceLoss(TverskyLoss):
    """The soft Dice loss ``1 - (2 I + smooth) / (P + Y + smooth)`` averaged over segments and classes (``ops.dice_loss``):
    ``TverskyLoss(alpha=0.5, beta=0.5, gamma=1, smooth=smooth / 2)`` bit for bit, with its other options."""

    def __init__(self, smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100):
        ops.check_tversky_options(0.5, 0.5, 1.0, smooth, "DiceLoss")
        super().__init__(0.5, 0.5, 1.0, smooth / 2.0, classes, per_image, present_only, ignore_index)

    def extra_repr(self):
        return (f"smooth={2.0 * self.smooth}, classes={self.classes}, per_image={self.per_image}, "
                f"present_only={self.present_only}, ignore_index={self.ignore_index}")


class FocalLoss(_Criterion):
    """The focal loss of Lin et al. (ICCV 2017) in its softmax form (``ops.focal_loss``): per pixel ``weight[y] (1 - s_y) **
    gamma (-log s_y)``, with the class weights, the ``ignore_index``, the reductions and the per-pixel confidence weight of
    ``CrossEntropyLoss`` (``set_pixel_weight``); ``gamma = 0`` is that cross entropy.  Conventions of ``CrossEntropyLoss``:
    the buffers keep their addresses and every option is a plain attribute (``plan.host_scalars``)."""

    _pointers = ("weight", "pixel_weight")
    _shapes = ("pixel_weight",)

    def __init__(self, gamma=2.0, weight=None, ignore_index=-100, reduction="mean"):
        super().__init__()
        ops.check_focal_options(gamma, reduction, "FocalLoss")
        self.register_buffer("weight", self._class_weight(weight))
        self.register_buffer("pixel_weight", None, persistent=False)
        self.gamma = float(gamma)
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self._refresh_pointers()

    set_pixel_weight = _Criterion._set_pixel_weight

    def forward(self, logits, labels):
        ops.check_focal_options(self.gamma, self.reduction, "FocalLoss")
        self._refresh_pointers()
        return ops.focal_loss(logits, labels.long(), gamma=self.gamma, weight=self.weight, ignore_index=self.ignore_index,
                              reduction=self.reduction, pixel_weight=self.pixel_weight)

    def extra_repr(self):
        return (f"gamma={self.gamma}, ignore_index={self.ignore_index}, reduction={self.reduction!r}, "
                f"weight={self.weight is not None}")


class CrossEntropyTverskyLoss(_Criterion):
    """``cross entropy + lam * Tversky loss`` - the usual pairing of a pixel loss with a region-overlap loss for imbalanced
    masks: ``ops.cross_entropy(logits, labels, weight=, ignore_index=, label_smoothing=)`` plus ``TverskyLoss(alpha, beta,
    gamma, smooth, classes, per_image, present_only, ignore_index)`` scaled by ``lam``, added by the library's kernels
    (``ops.fanout`` / ``ops.add_scalars``), so ``train_step`` replays one launch plan.  Built like
    ``CrossEntropyBoundaryLoss``: ``lam`` lives in the one-element device buffer ``lam_dev`` and is read by the kernel;
    ``set_lam(v)`` writes the buffer WITHOUT a new plan.  ``lam = 0`` is the cross entropy bit for bit.  The Tversky
    options are attributes of ``self.tversky``; a changed ``alpha`` records a new plan.

        crit = wnn.CrossEntropyTverskyLoss(lam=1.0, alpha=0.3, beta=0.7, classes=(1,)).to(device)
        loss = train_step(model, optimizer, images, masks, criterion=crit)
    """

    _pointers = ("weight", "lam_dev")

    def __init__(self, lam=1.0, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False, present_only=False,
                 weight=None, ignore_index=-100, label_smoothing=0.0):
        super().__init__()
        ops.check_cross_entropy_options("mean", label_smoothing)
        lam = self._check_lam(lam)
        self.register_buffer("weight", self._class_weight(weight))
        self.register_buffer("lam_dev", torch.tensor([lam], dtype=torch.float32), persistent=False)
        self.tversky = TverskyLoss(alpha, beta, gamma, smooth, classes, per_image, present_only, ignore_index)
        self.ignore_index = int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        self._refresh_pointers()

    @staticmethod
    def _check_lam(lam):
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= lam < float("inf"):
            raise ValueError(f"CrossEntropyTverskyLoss: lam {lam!r} must be a finite number >= 0")
        return float(lam)

    def set_lam(self, lam):
        """Write ``lam`` into the device buffer (a stream-ordered fill; the buffer keeps its address)."""
        self.lam_dev.fill_(self._check_lam(lam))
        return self

    def forward(self, logits, labels):
        ops.check_cross_entropy_options("mean", self.label_smoothing)
        self._refresh_pointers()
        labels = labels.long()
        self.tversky.ignore_index = self.ignore_index
        self.tversky.scale_dev = self.lam_dev
        a, b = ops.fanout(logits, 2)
        ce = ops.cross_entropy(a, labels, self.ignore_index, weight=self.weight, label_smoothing=self.label_smoothing)
        return ops.add_scalars(ce, self.tversky(b, labels))

    def extra_repr(self):
        return (f"{self.tversky.extra_repr()}, label_smoothing={self.label_smoothing}, weight={self.weight is not None}")


class SeededRegionGrowingLoss(_Criterion):
    """The seeding loss of deep seeded region growing (DSRG; Huang et al., CVPR 2018): the ``labels`` of a call are SEEDS - the
    few pixels a CAM is sure of, a value in [0,C) per seeded pixel and anything else where there is none
    (``PsuedoMasks.seeds_from_cam``) - and on every call the network's own prediction grows them: ``ops.softmax_channels`` of
    the detached logits, ``ops.seeded_region_growing`` with the thresholds ``thresh`` (a number, a ``(bg, fg)`` pair - the
    paper's 0.99 / 0.85 - or one number per class), ``ops.balanced_seed_weights`` and then the fused cross entropy against the
    grown labels, ``ops.cross_entropy(logits, grown, ignore_index, reduction="sum", pixel_weight=)`` (``balance="none"``:
    ``reduction="mean"`` with weights of one).  ``balance="fg_bg"`` is the paper's ``-1/|S_bg| sum log H - 1/|S_fg| sum log H``,
    averaged over the batch; ``"class"`` balances every class by itself.  The grown labels are constants, as in the paper: the
    gradient reaches the logits through the cross entropy only.  ``weight``: class weights of the cross entropy.

    Conventions of ``CrossEntropyLoss``: ``grown`` (int64 (B,H,W)), ``counts`` (int64 (B,C)), ``pixel_weight`` (float32) and
    ``thresh`` (float32 (C,)) are buffers of this object, filled by every call and allocated anew only when the shape changes,
    so the addresses a launch plan freezes stay put; every option and every address is a plain attribute, so
    ``plan.host_scalars`` puts them into the plan key and another ``balance`` records a new plan.  The thresholds live in the
    device buffer and are read by the kernel: ``set_thresh(...)`` writes it WITHOUT a new plan (a threshold schedule replays ONE
    plan).  Everything is a launch of the library without a host read.

    ``train_step`` clamps its masks to at most 1 as the reference does, so seeds that go through it mark "unseeded" with a
    NEGATIVE value (``seeds_from_cam(cam, lo, hi, ignore_index=-100)``); ``ignore_index`` here is what ``grown`` holds at the
    pixels nothing reached, any value outside [0,C).

        crit = wnn.SeededRegionGrowingLoss(thresh=(0.99, 0.85)).to(device)
        seeds = PsuedoMasks.seeds_from_cam(cam, 0.05, 0.6, ignore_index=-100)
        loss = train_step(model, optimizer, images, seeds, criterion=crit)
    """

    _pointers = ("weight", "pixel_weight", "grown", "counts", "thresh")
    _shapes = ("pixel_weight", "thresh")

    def __init__(self, thresh=(0.99, 0.85), balance="fg_bg", ignore_index=255, weight=None):
        super().__init__()
        ops.check_balance(balance, "SeededRegionGrowingLoss")
        ops.srg_thresholds(thresh, self._spec_len(thresh))  # (its type; the count is checked against C at the first call)
        self.register_buffer("weight", self._class_weight(weight))
        for name in ("pixel_weight", "grown", "counts", "thresh"):
            self.register_buffer(name, None, persistent=False)
        self._thresh_spec = [thresh]                       # (a list: not a host scalar of the plan key - the values live on the device)
        self.balance = balance
        self.ignore_index = int(ignore_index)
        self._refresh_pointers()

    @staticmethod
    def _spec_len(thresh):
        return len(thresh) if isinstance(thresh, (tuple, list)) else 2

    def set_thresh(self, thresh):
        """Write the thresholds into the device buffer (a stream-ordered copy; the buffer keeps its address)."""
        ops.srg_thresholds(thresh, self._spec_len(thresh) if self.thresh is None else self.thresh.numel())
        self._thresh_spec = [thresh]
        if self.thresh is not None:
            self._write_thresh()
        return self

    def _write_thresh(self):
        vals = ops.srg_thresholds(self._thresh_spec[0], self.thresh.numel())
        self.thresh.copy_(torch.tensor(vals, dtype=torch.float32))

    def forward(self, logits, labels):
        # (options may have been assigned since the constructor checked them)
        ops.check_balance(self.balance, "SeededRegionGrowingLoss")
        if not torch.is_tensor(logits) or logits.dim() != 4:
            raise ValueError("SeededRegionGrowingLoss: logits must be a (B,C,H,W) tensor")
        B, Cc, H, W = logits.shape
        if self.thresh is None or self.thresh.numel() != Cc or self.thresh.device != logits.device:
            ops.srg_thresholds(self._thresh_spec[0], Cc)
            self.thresh = torch.empty(Cc, device=logits.device, dtype=torch.float32)
            self._write_thresh()
        if self.pixel_weight is None or tuple(self.pixel_weight.shape) != (B, H, W) or self.pixel_weight.device != logits.device:
            self.pixel_weight = torch.empty((B, H, W), device=logits.device, dtype=torch.float32)
        bufs = {"grown": self.grown, "counts": self.counts}
        ops.seeded_region_growing(ops.softmax_channels(logits.detach()), labels.long(), self.thresh,
                                  ignore_index=self.ignore_index, out=bufs)
        self._adopt(bufs, {"grown": "grown", "counts": "counts"})
        ops.balanced_seed_weights(self.grown, self.counts, balance=self.balance, out=self.pixel_weight)
        return ops.cross_entropy(logits, self.grown, self.ignore_index, weight=self.weight,
                                 reduction="mean" if self.balance == "none" else "sum", pixel_weight=self.pixel_weight)

    def extra_repr(self):
        return (f"thresh={self._thresh_spec[0]!r}, balance={self.balance!r}, ignore_index={self.ignore_index}, "
                f"weight={self.weight is not None}")


class ConsistencyLoss(_Criterion):
    """The consistency loss of ``ops.consistency_loss`` between the student's logits and a teacher prediction this object
    holds - the consistency cost of a mean teacher, FixMatch's confident pseudo-targets (``kind="hard"``, ``tau``) or an
    equivariance term - shaped as an ``extra_loss`` of ``train_step``: ``forward(student_logits, images=None)``.

    ``set_teacher(teacher, rows=None)`` copies the teacher's (B,C,h,w) prediction - and the (B,8) rows that map the student's
    pixel grid to the teacher's (``augment.relative_rows``; None: same grid, direct read) - into buffers this object owns,
    allocated anew only when a shape changes, so the addresses a launch plan freezes stay put while the contents change every
    step.  ``tau``, ``lam`` and the temperature live in ONE three-float device buffer (``knobs``) the kernel reads:
    ``set_tau`` / ``set_lam`` / ``set_temperature`` write it WITHOUT a new plan (a ramp of the consistency weight is a ``set_lam``
    per step).  ``kind``, ``teacher_is``, ``normalize``, ``fill``, every address and the shapes are plain attributes, so
    ``plan.host_scalars`` puts them into the plan key: another ``kind`` records another plan.  ``counts`` (int64 (2,), on the
    device) holds ``(pixels inside, pixels counted)`` of the last call.

        cons = wnn.ConsistencyLoss(kind="kl", tau=0.7, lam=0.0).to(device)
        cons.set_teacher(teacher_logits, rows); cons.set_lam(ramp(step))
        loss = train_step(model, optimizer, view, labels, extra_loss=cons)
    """

    _pointers = ("teacher", "rows", "knobs", "counts", "pixel_weight")
    _shapes = ("teacher", "pixel_weight")

    def __init__(self, kind="kl", temperature=1.0, tau=0.0, lam=1.0, normalize="all", fill="ignore", teacher_is="logits"):
        super().__init__()
        self._check(kind, teacher_is, normalize, fill, temperature, tau, lam)
        self.kind, self.teacher_is, self.normalize, self.fill = kind, teacher_is, normalize, fill
        for name in ("teacher", "rows", "pixel_weight"):
            self.register_buffer(name, None, persistent=False)
        self.register_buffer("knobs", torch.tensor([float(tau), float(lam), float(temperature)], dtype=torch.float32),
                             persistent=False)
        self.register_buffer("counts", torch.zeros(2, dtype=torch.int64), persistent=False)
        self._refresh_pointers()

    @staticmethod
    def _check(kind, teacher_is, normalize, fill, temperature=1.0, tau=0.0, lam=1.0):
        for v, table, what in ((kind, ops.CONSISTENCY_KINDS, "kind"), (teacher_is, ops.CONSISTENCY_TEACHER, "teacher_is"),
                               (normalize, ops.CONSISTENCY_NORMALIZE, "normalize"), (fill, ops.AUGMENT_FILLS, "fill")):
            if not isinstance(v, str) or v not in table:
                raise ValueError(f"ConsistencyLoss: {what} {v!r}: one of {sorted(table)}")
        if not ops._knob_ok(temperature, 0.0, None, True):
            raise ValueError(f"ConsistencyLoss: temperature {temperature!r} must be a finite number > 0")
        if not ops._knob_ok(tau, 0.0, 1.0):
            raise ValueError(f"ConsistencyLoss: tau {tau!r} must be a number in [0, 1]")
        if not ops._knob_ok(lam):
            raise ValueError(f"ConsistencyLoss: lam {lam!r} must be a finite number")

    def _own(self, name, t):
        """Copy ``t`` into the buffer ``name`` (allocated anew only when shape or device change); None drops it."""
        if t is None:
            setattr(self, name, None)
            return
        cur = getattr(self, name)
        if cur is None or cur.shape != t.shape or cur.device != t.device:
            cur = torch.empty(t.shape, device=t.device, dtype=torch.float32)
            setattr(self, name, cur)
        cur.copy_(t.detach())

    def set_teacher(self, teacher, rows=None):
        if not torch.is_tensor(teacher) or teacher.dim() != 4:
            raise ValueError("ConsistencyLoss.set_teacher: teacher must be a (B,C,h,w) tensor")
        if rows is not None and (not torch.is_tensor(rows) or tuple(rows.shape) != (teacher.shape[0], 8)):
            raise ValueError(f"ConsistencyLoss.set_teacher: rows must be a {(teacher.shape[0], 8)} tensor or None")
        for t, what in ((teacher, "teacher"), (rows, "rows")):              # (the copy below would cast silently)
            if t is not None and t.dtype != torch.float32:
                raise ValueError(f"ConsistencyLoss.set_teacher: {what} must be float32, got {t.dtype}")
        self._own("teacher", teacher)
        self._own("rows", rows)
        self._refresh_pointers()
        return self

    set_pixel_weight = _Criterion._set_pixel_weight

    def set_tau(self, tau):
        self._check(self.kind, self.teacher_is, self.normalize, self.fill, tau=tau)
        self.knobs[0:1].fill_(float(tau))           # a stream-ordered fill; the buffer keeps its address
        return self

    def set_lam(self, lam):
        self._check(self.kind, self.teacher_is, self.normalize, self.fill, lam=lam)
        self.knobs[1:2].fill_(float(lam))
        return self

    def set_temperature(self, temperature):
        self._check(self.kind, self.teacher_is, self.normalize, self.fill, temperature=temperature)
        self.knobs[2:3].fill_(float(temperature))
        return self

    def forward(self, student_logits, images=None):
        # (options may have been assigned since the constructor checked them)
        self._check(self.kind, self.teacher_is, self.normalize, self.fill)
        if self.teacher is None:
            raise ValueError("ConsistencyLoss: set_teacher(teacher, rows) before the loss is taken")
        self._refresh_pointers()
        k = self.knobs
        return ops.consistency_loss(student_logits, self.teacher, self.rows, kind=self.kind, teacher_is=self.teacher_is,
                                    temperature=k[2:3], tau=k[0:1], lam=k[1:2], normalize=self.normalize, fill=self.fill,
                                    pixel_weight=self.pixel_weight, counts=self.counts)

    def extra_repr(self):
        return (f"kind={self.kind!r}, teacher_is={self.teacher_is!r}, normalize={self.normalize!r}, fill={self.fill!r}, "
                f"teacher={None if self.teacher is None else tuple(self.teacher.shape)}")


class PAMR(nn.Module):
    """Pixel-adaptive mask refinement (Araslanov & Roth, CVPR 2020) as a module without parameters: ``forward(images,
    scores)`` is ``ops.pamr(images, scores, num_iter, dilations)`` - scores (B,C,H,W) propagated ``num_iter`` times over
    the dilated 3 x 3 rings of every pixel with weights from the local contrast of images (B,K,H,W).  Not differentiable:
    the result has no ``grad_fn`` (the refiner of single-stage weakly-supervised segmentation sits behind a stop-gradient).

        refine = wnn.PAMR(num_iter=10)
        masks = ops.pamr_labels(refine(images, probs.detach()), min_conf=0.6)       # int64, 255 where unsure
        loss = train_step(model, optimizer, images, masks, criterion=wnn.CrossEntropyLoss(ignore_index=255))
    """

    def __init__(self, num_iter=10, dilations=ops.PAMR_DILATIONS):
        super().__init__()
        if isinstance(num_iter, bool) or not isinstance(num_iter, int) or num_iter < 0:
            raise ValueError(f"PAMR: num_iter {num_iter!r} must be an int >= 0")
        self.dilations, _ = ops._pamr_dilations(dilations)
        self.num_iter = num_iter

    def forward(self, images, scores):
        return ops.pamr(images, scores, self.num_iter, self.dilations)

    def extra_repr(self):
        return f"num_iter={self.num_iter}, dilations={self.dilations}"


class Superpixels(nn.Module):
    """Integer SLIC superpixels (``ops.slic``; the reference has no such step) as a module without parameters:
    ``forward(images)`` returns ``(segments, n_segments)`` for uint8 (B,3,H,W) device images, or for float images normalised with
    the ImageNet constants, which go through ``ops.slic_quantize`` first.  ``snap(images, scores)`` replaces every pixel of the
    float32 (B,C,H,W) ``scores`` by its superpixel's mean (``ops.superpixel_snap``), ``vote(images, labels, num_classes)`` every
    pixel of the int64 (B,H,W) ``labels`` by its superpixel's majority label (``ops.superpixel_vote``).  Not differentiable: the
    results have no ``grad_fn``.

        sp = wnn.Superpixels(step=16)
        cam = sp.snap(images, cam[:, None])[:, 0]                 # a blurry CAM snapped to image edges
        masks = sp.vote(images, masks, num_classes=2)             # a pseudo mask denoised without any learning
    """

    def __init__(self, step, compactness=10, num_iter=10, min_size=None):
        super().__init__()
        self.step, self.compactness, self.num_iter, self.min_size = ops.check_slic_options(step, compactness, num_iter, min_size,
                                                                                           name="Superpixels")

    def _images(self, images):
        return ops.slic_quantize(images) if torch.is_tensor(images) and images.is_floating_point() else images

    def max_segments(self, images):
        return ops.slic_max_segments(images.shape[-2], images.shape[-1], self.step, self.min_size)

    def forward(self, images):
        return ops.slic(self._images(images), self.step, self.compactness, self.num_iter, self.min_size)

    def snap(self, images, scores):
        segments, _ = self.forward(images)
        return ops.superpixel_snap(scores, segments, self.max_segments(images))

    def vote(self, images, labels, num_classes, ignore_index=255):
        segments, _ = self.forward(images)
        return ops.superpixel_vote(labels, segments, self.max_segments(images), num_classes, ignore_index)

    def extra_repr(self):
        return f"step={self.step}, compactness={self.compactness}, num_iter={self.num_iter}, min_size={self.min_size}"


class AffinityLoss(nn.Module):
    """AffinityNet's pair loss (Ahn & Kwak, CVPR 2018; ``ops.affinity_loss``) as a module without parameters:
    ``forward(feat, labels)`` for float32 features (B,D,h,w) and int64 labels (B,h,w) at the feature size - 0 background, > 0
    a class, ``ignore_index`` unsure (``affinity_labels_from_cam``).  ``weights`` are those of the bg-positive, fg-positive
    and negative terms.  A plain module: not one of the segmentation criteria ``train_step`` takes."""

    def __init__(self, radius=5, ignore_index=255, weights=ops.AFFINITY_WEIGHTS):
        super().__init__()
        ops.check_affinity_options(radius, weights=weights, name="AffinityLoss")
        self.radius, self.ignore_index, self.weights = radius, int(ignore_index), tuple(float(v) for v in weights)

    def forward(self, feat, labels):
        return ops.affinity_loss(feat, labels, radius=self.radius, ignore_index=self.ignore_index, weights=self.weights)

    def extra_repr(self):
        return f"radius={self.radius}, ignore_index={self.ignore_index}, weights={self.weights}"


class RandomWalk(nn.Module):
    """AffinityNet's CAM propagation as a module without parameters: ``forward(feat, scores)`` is
    ``ops.affinity_random_walk(feat, scores, radius=, beta=, num_iter=)`` - scores (B,C,h,w) walked ``num_iter`` steps under
    the transition weights of features (B,D,h,w).  Not differentiable: the result has no ``grad_fn``."""

    def __init__(self, radius=5, beta=8.0, num_iter=256):
        super().__init__()
        ops.check_affinity_options(radius, beta=beta, num_iter=num_iter, name="RandomWalk")
        self.radius, self.beta, self.num_iter = radius, float(beta), num_iter

    def forward(self, feat, scores):
        return ops.affinity_random_walk(feat, scores, radius=self.radius, beta=self.beta, num_iter=self.num_iter)

    def extra_repr(self):
        return f"radius={self.radius}, beta={self.beta}, num_iter={self.num_iter}"


class PrototypeContrastLoss(nn.Module):
    """Pixel-to-prototype contrast (Du et al., CVPR 2022; Wang et al., ICCV 2021; ``ops.prototype_contrast_loss``) as a module
    without parameters: ``forward(feat, labels)`` for float32 features (B,D,h,w) and int64 labels (B,h,w) in [0, num_classes) or
    ``ignore_index``.  The prototypes are pooled from the DETACHED features (``ops.class_prototypes``, unit vectors) into the
    module's own buffers - ``source='batch'``: one set over the batch, ``'image'``: one per image, ``'bank'``: the batch's set is
    first folded into a moving average over the calls (``ops.prototype_ema_`` with ``momentum``; ``bank`` (K,D), ``count`` (K,)
    int64, registered buffers: they are in the state dict and move with ``.to()``; ``reset()`` empties both) and the bank is what the
    pixels are compared with.  The classes present are those with ``mass >
    0`` (``count > 0`` for the bank); then the fused loss, mean over the counted pixels.  The gradient flows into ``feat`` only.
    A plain module: not one of the segmentation criteria ``train_step`` takes."""

    SOURCES = ("batch", "image", "bank")

    def __init__(self, num_classes, temperature=0.1, source="batch", momentum=0.99, ignore_index=255):
        super().__init__()
        ops.check_prototype_options(num_classes=num_classes, temperature=temperature, momentum=momentum, name="PrototypeContrastLoss")
        if source not in self.SOURCES:
            raise ops.WsdlError(f"PrototypeContrastLoss: source {source!r}: 'batch', 'image' or 'bank'")
        self.num_classes, self.temperature, self.source = num_classes, float(temperature), source
        self.momentum, self.ignore_index = float(momentum), int(ignore_index)
        # registered buffers, filled at the first call (the channel count is the features'): ``bank`` and ``count`` are part of the
        # state dict and move with ``.to()``; ``proto`` and ``mass`` are the last call's scratch and are not saved
        self.register_buffer("bank", None)
        self.register_buffer("count", None)
        self.register_buffer("proto", None, persistent=False)
        self.register_buffer("mass", None, persistent=False)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a bank saved after its first call loads into a module that has not been called yet
        for name in ("bank", "count"):
            saved = state_dict.get(prefix + name)
            if saved is not None and (getattr(self, name) is None or getattr(self, name).shape != saved.shape):
                setattr(self, name, torch.empty_like(saved, device=saved.device if getattr(self, name) is None else getattr(self, name).device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def reset(self):
        """Empty the bank: every class takes the next prototype it sees as it is."""
        if self.bank is not None:
            ops.memset_zero(self.bank)
            ops.memset_zero(self.count)

    def _make_buffers(self, S, D, device):
        if self.proto is None or tuple(self.proto.shape) != (S, self.num_classes, D) or self.proto.device != device:
            self.proto = torch.zeros(S, self.num_classes, D, device=device)
            self.mass = torch.zeros(S, self.num_classes, device=device)
        if self.source == "bank" and (self.bank is None or self.bank.shape[1] != D or self.bank.device != device):
            self.bank = torch.zeros(self.num_classes, D, device=device)
            self.count = torch.zeros(self.num_classes, dtype=torch.int64, device=device)

    def forward(self, feat, labels):
        per_image = self.source == "image"
        ops.check_prototype_options(feat=feat, labels=labels, name="PrototypeContrastLoss")
        self._make_buffers(feat.shape[0] if per_image else 1, feat.shape[1], feat.device)
        ops.class_prototypes(feat.detach(), labels, self.num_classes, per_image=per_image, ignore_index=self.ignore_index,
                             out=(self.proto, self.mass))
        if self.source == "bank":
            ops.prototype_ema_(self.bank, self.count, self.proto, self.mass, self.momentum)
            proto, present = self.bank[None], self.count[None] > 0
        else:
            proto, present = self.proto, self.mass > 0
        return ops.prototype_contrast_loss(feat, proto, labels, temperature=self.temperature, present=present,
                                           ignore_index=self.ignore_index)

    def extra_repr(self):
        return (f"num_classes={self.num_classes}, temperature={self.temperature}, source={self.source!r}, momentum={self.momentum}, "
                f"ignore_index={self.ignore_index}")


class PathAffinityLoss(nn.Module):
    """IRN's boundary loss (Ahn, Cho & Kwak, CVPR 2019; ``ops.path_affinity_loss``) as a module without parameters:
    ``forward(edge_logits, labels)`` for the float32 logits (B,1,h,w) or (B,h,w) of a boundary head and int64 labels (B,h,w) at
    the logit size - 0 background, > 0 a class, ``ignore_index`` unsure (``affinity_labels_from_cam``).  ``weights`` are those of
    the bg-positive, fg-positive and negative terms.  A plain module: not one of the segmentation criteria ``train_step`` takes."""

    def __init__(self, radius=5, ignore_index=255, weights=ops.AFFINITY_WEIGHTS):
        super().__init__()
        ops.check_path_affinity_options(radius, weights=weights, name="PathAffinityLoss")
        self.radius, self.ignore_index, self.weights = radius, int(ignore_index), tuple(float(v) for v in weights)

    def forward(self, edge_logits, labels):
        return ops.path_affinity_loss(edge_logits, labels, radius=self.radius, ignore_index=self.ignore_index, weights=self.weights)

    def extra_repr(self):
        return f"radius={self.radius}, ignore_index={self.ignore_index}, weights={self.weights}"


class EdgeRandomWalk(nn.Module):
    """IRN's CAM propagation as a module without parameters: ``forward(edge, scores)`` is ``ops.edge_random_walk(edge, scores,
    radius=, beta=, num_iter=)`` - scores (B,C,h,w) damped by ``1 - edge`` and walked ``num_iter`` steps under the path affinities
    of the boundary map (B,1,h,w) or (B,h,w).  Not differentiable: the result has no ``grad_fn``."""

    def __init__(self, radius=5, beta=10.0, num_iter=256):
        super().__init__()
        ops.check_path_affinity_options(radius, beta=beta, num_iter=num_iter, name="EdgeRandomWalk")
        self.radius, self.beta, self.num_iter = radius, float(beta), num_iter

    def forward(self, edge, scores):
        return ops.edge_random_walk(edge, scores, radius=self.radius, beta=self.beta, num_iter=self.num_iter)

    def extra_repr(self):
        return f"radius={self.radius}, beta={self.beta}, num_iter={self.num_iter}"
