"""SegmentationModel (DeepLabV3-ResNet50) on the HIP path.

The reference has no class of this name: it builds
``torchvision.models.segmentation.deeplabv3_resnet50(pretrained=True)`` and swaps
``classifier[4] = nn.Conv2d(256, 2, 1)`` (TraditionalModel/SegmentationModel.py:85-88,
AlternatingDirectionCutLoss.py:784-787), always calling ``model(images)['out']``.  ``SegmentationModel``
keeps that call surface - ``forward(x)`` returns an OrderedDict with 'out' (and 'aux' while the aux
head exists) - and torchvision's module / state_dict names (backbone.*, classifier.0.convs.*,
classifier.0.project.*, classifier.{1,2,4}.*, aux_classifier.{0,1,4}.*).

Architecture (published torchvision definition): ResNet-50 backbone with
``replace_stride_with_dilation=[False, True, True]`` (output stride 8), DeepLabHead = ASPP(2048,
rates 12/24/36, + image pooling) -> 1x1 project + Dropout(0.5) -> 3x3 -> 1x1, FCNHead aux classifier
on layer3 (computed every forward as in the reference, unused by its losses), bilinear up-sampling to
the input size.  Convolutions, BatchNorm, pooling, dropout, resampling and the loss are HIP kernels.

``train_step`` is one iteration of the reference's training loop (SegmentationModel.py:96-113 /
AlternatingDirectionCutLoss.py:693-703): clamp masks to {0,1}, forward, CrossEntropy, backward, Adam.
"""
from collections import OrderedDict

import os

import torch
import torch.nn as nn

from .. import nn as wnn
from .. import ops
from .. import plan
from ..augment import Mix
from ..optim import FlatAdam, FlatAdamW, FlatSGD
from .ExtraUtilities import compute_iou_and_acc


def _cbr(cin, cout, k, dilation=1):
    return [wnn.Conv2d(cin, cout, k, padding=0 if k == 1 else dilation, dilation=dilation), wnn.BatchNorm2d(cout),
            wnn.ReLU()]


class _ASPPPooling(wnn.FusedSequential):
    def __init__(self, cin, cout):
        super().__init__(wnn.GlobalAvgPool(), *_cbr(cin, cout, 1))

    def forward(self, x):
        size = x.shape[-2:]
        return ops.bilinear_resize(super().forward(x), size)


_ASPP_IN_PLACE = os.environ.get("WSDL_ASPP_IN_PLACE", "1") != "0"     # A/B: 0 = plane copies of all five branches


class ASPP(nn.Module):
    def __init__(self, cin=2048, rates=(12, 24, 36), cout=256):
        super().__init__()
        branches = [wnn.FusedSequential(*_cbr(cin, cout, 1))]
        branches += [wnn.FusedSequential(*_cbr(cin, cout, 3, r)) for r in rates]
        branches.append(_ASPPPooling(cin, cout))
        self.convs = nn.ModuleList(branches)
        self.project = wnn.FusedSequential(*_cbr(len(branches) * cout, cout, 1), wnn.Dropout(0.5))

    def forward(self, x):
        # x feeds five branches: chain it through the four conv nodes (ops.conv_bn_act passthrough) so that the five
        # input gradients are summed inside the dgrad epilogues instead of by four 134 MB autograd adds
        branches = list(self.convs)
        if x.is_cuda and all(b[1].training for b in branches[:-1]) and _ASPP_IN_PLACE:
            # train mode: the BatchNorm kernels of the four convolution branches write straight into their channel slices of
            # the concatenation (and publish into ONE amax slot); only the pooling branch is copied in
            B, _, H, W = x.shape
            cs = [b[0].out_channels for b in branches[:-1]]
            cat = torch.empty(B, self.project[0].in_channels, H, W, device=x.device, dtype=torch.float32)
            slot = ops.amax_slot(x.device) if ops.CONV_ARITH[0] == 1 else None
            outs, off = [], 0
            convs = [b[0] for b in branches[:-1]]
            bns = [b[1] for b in branches[:-1]]
            if (ops.ASPP_MULTI[0] and torch.is_grad_enabled() and x.requires_grad and len(set(cs)) == 1
                    and all(m.stride == 1 and m.bias is None and m.weight.requires_grad and m.padding == m.dilation * (m.kernel_size - 1) // 2
                            and getattr(m.weight, "_wsdl_grad_sink", None) is not None for m in convs)
                    and all(bn.weight.requires_grad and getattr(bn.weight, "_wsdl_grad_sink", None) is not None
                            and bn.momentum == bns[0].momentum and bn.eps == bns[0].eps for bn in bns)
                    and ops.dgrad_multi_ok(len(convs), tuple(x.shape), cs[0])):
                # the four convolution branches as ONE node: their input gradients are one launch (ops._ConvBNBranches)
                holders = []
                for c in cs:
                    holders.append([cat[:, off:off + c], slot])
                    off += c
                for bn in bns:
                    bn._pending_steps += 1
                res = ops.conv_bn_branches(x, list(zip(convs, bns, holders)), bns[0].momentum, bns[0].eps)
                outs, x = list(res[:-1]), res[-1]
                outs.append(branches[-1](x))
                return self.project(ops.concat_into(cat, slot, outs))
            for b, c in zip(branches[:-1], cs):
                y, x = wnn.conv_bn(x, b[0], b[1], True, passthrough=True, out_holder=[cat[:, off:off + c], slot])
                outs.append(y)
                off += c
            outs.append(branches[-1](x))
            return self.project(ops.concat_into(cat, slot, outs))
        outs = []
        for b in branches[:-1]:
            y, x = wnn.conv_bn(x, b[0], b[1], True, passthrough=True)
            outs.append(y)
        outs.append(branches[-1](x))
        return self.project(ops.concat_channels(outs))


class _Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.bn1, (self.layer1, self.layer2, self.layer3, self.layer4) = \
            wnn.make_resnet50_stages((False, True, True))
        self.relu, self.maxpool = wnn.ReLU(), wnn.MaxPool3x3s2()

    def forward(self, x):
        x = self.maxpool(wnn.conv_bn(x, self.conv1, self.bn1, True))
        x = self.layer2(self.layer1(x))
        f3 = self.layer3(x)
        return OrderedDict(out=self.layer4(f3), aux=f3)


_AUX_ON_SIDE_STREAM = os.environ.get("WSDL_AUX_SIDE", "1") != "0"


class _Outputs(OrderedDict):
    """The result dict of ``forward``.  In eval mode the aux head - which no caller of the reference ever reads
    ("computed every forward, unused by every loss") and which has no side effect there (eval-mode
    BatchNorm, no dropout) - is computed when 'aux' is first looked at instead of on every forward: refine_pseudo_mask
    and evaluate_model only take ['out'].  In train mode it is computed eagerly, as torchvision does (its BatchNorm
    running statistics move)."""

    def __init__(self):
        super().__init__()
        self._lazy = {}

    def _resolve(self, key):
        fn = self._lazy.pop(key, None)
        if fn is not None:
            super().__setitem__(key, fn())

    def __getitem__(self, key):
        self._resolve(key)
        return super().__getitem__(key)

    def __contains__(self, key):
        return key in self._lazy or super().__contains__(key)

    def _all(self):
        for k in list(self._lazy):
            self._resolve(k)

    def keys(self):
        self._all()
        return super().keys()

    def values(self):
        self._all()
        return super().values()

    def items(self):
        self._all()
        return super().items()

    def __iter__(self):
        self._all()
        return super().__iter__()

    def __len__(self):
        return super().__len__() + len(self._lazy)

    # every read access of the dict API resolves the lazy entries first: ``out.get('aux')`` must not answer None for a
    # key ``'aux' in out`` reports (torchvision returns a plain OrderedDict)
    def get(self, key, default=None):
        return self[key] if key in self else default

    def pop(self, key, *default):
        self._resolve(key)
        return super().pop(key, *default)

    def popitem(self, last=True):
        self._all()
        return super().popitem(last)

    def setdefault(self, key, default=None):
        if key in self:
            return self[key]
        super().__setitem__(key, default)
        return default

    def __setitem__(self, key, value):
        if getattr(self, "_lazy", None):
            self._lazy.pop(key, None)
        super().__setitem__(key, value)

    def __delitem__(self, key):
        if self._lazy.pop(key, None) is None:
            super().__delitem__(key)

    def copy(self):
        self._all()
        return OrderedDict(super().items())

    def __eq__(self, other):
        self._all()
        return super().__eq__(other)

    def __repr__(self):
        self._all()
        return super().__repr__()


class SegmentationModel(nn.Module):
    def __init__(self, num_classes=2, aux_loss=True, aux_classes=21):
        super().__init__()
        self.backbone = _Backbone()
        self.classifier = wnn.FusedSequential(ASPP(), *_cbr(256, 256, 3, 1), wnn.Conv2d(256, num_classes, 1, bias=True))
        self.aux_classifier = None
        if aux_loss:
            self.aux_classifier = wnn.FusedSequential(*_cbr(1024, 256, 3, 1), wnn.Dropout(0.1),
                                                      wnn.Conv2d(256, aux_classes, 1, bias=True))
        for m in self.modules():
            if isinstance(m, wnn.Conv2d) and m.bias is not None:
                m.reset_parameters()

    # The train-mode aux head runs on the side stream (forward below) and writes its BatchNorm running statistics there.
    # A training step joins that stream before Adam; a train-mode forward WITHOUT a step (BatchNorm recalibration, a
    # loss-only validation pass) does not - so every place that reads those buffers on another stream joins first.
    def _join_aux(self):
        ev = self.__dict__.get("_aux_event")
        if ev is not None:
            self.__dict__["_aux_event"] = None
            if not torch.cuda.is_current_stream_capturing():
                ev.wait()      # the event sits right behind the aux head: not the whole side stream

    def train(self, mode=True):
        self._join_aux()
        return super().train(mode)

    def state_dict(self, *args, **kwargs):
        self._join_aux()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._join_aux()
        return super().load_state_dict(*args, **kwargs)

    def head_logits(self, x):
        """The classifier's output BEFORE the final ``bilinear_resize`` of ``forward``: (B, C, h/8, w/8), the stride-8 logits
        ``ops.multiscale_fuse`` resamples itself (``bilinear_resize(head_logits(x), x.shape[-2:])`` is ``forward(x)['out']``).  The
        aux head is not computed."""
        self._join_aux()
        return self.classifier(self.backbone(x)["out"])

    def forward(self, x):
        size = x.shape[-2:]
        self._join_aux()              # a previous forward's aux head may still be writing the statistics read / written now
        feats = self.backbone(x)
        res = _Outputs()
        if self.aux_classifier is not None and self.training and x.is_cuda and _AUX_ON_SIDE_STREAM and \
                not torch.cuda.is_current_stream_capturing():
            # Train mode computes the aux head on every forward, as torchvision does (its BatchNorm statistics move), and
            # no loss of the reference reads it: it runs on the side stream - idle during forward - beside the main head
            # instead of after it; whoever does look at ['aux'] joins first.
            f3 = feats["aux"]
            side = ops.side_stream(x.device)
            ops.stream_wait(side, ops.raw_stream(x.device))
            ops.cross_stream_use(f3, side)
            with torch.cuda.stream(side):
                aux_out = ops.bilinear_resize(self.aux_classifier(f3), size)
            ev = self.__dict__.get("_aux_event_obj")        # one event, re-recorded by every forward (part of a launch plan)
            if ev is None:
                ev = self.__dict__["_aux_event_obj"] = ops.Event()
            ev.record(side)
            self.__dict__["_aux_event"] = ev

            def joined():
                ops.stream_wait(ops.raw_stream(x.device), side)
                return aux_out
            res["out"] = ops.bilinear_resize(self.classifier(feats["out"]), size)
            res._lazy["aux"] = joined
            return res
        res["out"] = ops.bilinear_resize(self.classifier(feats["out"]), size)
        if self.aux_classifier is not None:
            f3 = feats["aux"]
            if self.training:
                res["aux"] = ops.bilinear_resize(self.aux_classifier(f3), size)
            else:
                grad = torch.is_grad_enabled()

                def aux():
                    with torch.set_grad_enabled(grad):
                        return ops.bilinear_resize(self.aux_classifier(f3), size)
                res._lazy["aux"] = aux
        return res


def build_segmentation_model(num_classes=2, aux_loss=True):
    """The reference's construction: 21-class DeepLabV3 with aux head, classifier[4] swapped."""
    return SegmentationModel(num_classes=num_classes, aux_loss=aux_loss, aux_classes=21)


def resolve_criterion(criterion):
    """What a reference-style ``criterion`` object means on the HIP path.  ``nn.CrossEntropyLoss()`` (the only criterion
    the reference constructs: SegmentationModel.py:90, AlternatingDirectionCutLoss.py:789) maps onto the fused
    softmax-cross-entropy kernel with its ``ignore_index``, its class ``weight`` (moved to the logits' device once, by the
    caller: a host tensor raises) and ``reduction`` 'mean' or 'sum'.  ``reduction='none'`` raises: a training step needs a
    scalar.  ``label_smoothing`` on torch's class raises too - kept from the time the kernel had no smoothing; the
    project's own ``weaklysuperviseddl_amd.nn.CrossEntropyLoss`` has it (and pixel weights), and being a callable it is
    applied as it is, like any other callable on ``(outputs, masks)``."""
    if criterion is None:
        return lambda o, m: ops.cross_entropy(o, m.long())
    if isinstance(criterion, nn.CrossEntropyLoss):
        if getattr(criterion, "label_smoothing", 0.0) != 0.0:
            raise ValueError("train_step: label smoothing is not taken from torch.nn.CrossEntropyLoss; use "
                             "weaklysuperviseddl_amd.nn.CrossEntropyLoss(label_smoothing=...), which runs it in the kernel")
        if criterion.reduction not in ("mean", "sum"):
            raise ValueError(f"train_step: nn.CrossEntropyLoss(reduction={criterion.reduction!r}): a training step needs a "
                             "scalar loss ('mean' or 'sum')")
        ign, weight, reduction = int(criterion.ignore_index), criterion.weight, criterion.reduction
        if weight is None and reduction == "mean":
            return lambda o, m: ops.cross_entropy(o, m.long(), ign)
        return lambda o, m: ops.cross_entropy(o, m.long(), ign, weight=weight, reduction=reduction)
    if callable(criterion):
        return criterion
    raise TypeError(f"criterion: expected nn.CrossEntropyLoss, a callable or None, got {type(criterion).__name__}")


_ONES = {}


def _one(device):
    """The gradient of the loss with respect to itself, allocated once (``loss.backward()`` fills a new tensor with a kernel
    of the tensor library on every call - which a launch plan would not see)."""
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones((), device=device, dtype=torch.float32)
    return t


def train_step(model, optimizer, images, masks, extra_loss=None, loss_fn="cross_entropy", criterion=None, *,
               ignore_label=None):
    """One training iteration; returns the (device) loss tensor, no host synchronisation.  ``loss_fn``: 'cross_entropy' or
    'lovasz_softmax' (reference SegmentationModel.py:65,103-107), or 'lovasz_hinge': the binary Lovasz hinge of the
    reference's loss file (LossFunctions/Lovasz-Softmax_Loss.py:71-104) on the logit difference z1 - z0, per image;
    ``criterion``: a reference-style loss object instead (``resolve_criterion``).

    ``ignore_label`` (default None: nothing changes): a label the ``loss_fn`` losses leave out - ``ignore=`` of the two
    Lovasz losses, ``ignore_index`` of the cross entropy (a ``criterion`` keeps its own).  Batches augmented with
    ``fill="ignore"`` carry -100 where the warp left the source: the cross entropy ignores that value by default, with or
    without a ``criterion``, but a Lovasz ``loss_fn`` needs ``ignore_label=-100``.  ``fill="reflect"`` pads nothing and
    needs nothing - the mode to use with the NCut and boundary terms (``extra_loss``), which would otherwise see an edge
    at the pad border.

    On the device, in train mode and outside data parallelism the iteration is issued as ONE host call from its third
    occurrence on (``plan.PlannedTrainStep``: the launches of an eager iteration recorded behind the C ABI, verified to
    reproduce it bit for bit, then replayed); WSDL_PLAN_STEP=0 keeps every iteration eager."""
    if isinstance(optimizer, FlatAdam) and images.is_cuda and plan.PLAN_STEP[0]:
        tag = (plan.loss_tag(extra_loss), loss_fn, plan.loss_tag(criterion))
        if ignore_label is not None:
            tag += (int(ignore_label),)
        weight = getattr(criterion, "weight", None)
        if torch.is_tensor(weight):                    # a replaced class-weight tensor is another plan; values changed in place are read by replays
            tag += (weight.data_ptr(),)
        st = plan.planned_step_for(model, optimizer,
                                   lambda i, m: _train_step_eager(model, optimizer, i, m, extra_loss, loss_fn, criterion,
                                                                  ignore_label), tag)
        # host scalars inside the loss objects (weights, window sizes, sigmas) are kernel arguments a plan freezes: part of its key
        st.loss_scalars = (plan.host_scalars(extra_loss), plan.host_scalars(criterion)) if (extra_loss is not None or criterion is not None) else None
        return st(images, masks)
    return _train_step_eager(model, optimizer, images, masks, extra_loss, loss_fn, criterion, ignore_label)


def _train_step_eager(model, optimizer, images, masks, extra_loss=None, loss_fn="cross_entropy", criterion=None,
                      ignore_label=None):
    masks = ops.clamp_max_labels(masks, 1)
    with ops.prof_range("train_step/forward"):
        outputs = model(images)["out"]
    with ops.prof_range("train_step/loss"):
        outputs_x = outputs
        if extra_loss is not None and outputs.is_cuda:
            # two consumers of the logits: their gradients are summed by the library (ops.fanout), not by the autograd
            # engine's own add kernel - which a launch plan would not see
            outputs, outputs_x = ops.fanout(outputs, 2)
        if criterion is not None:
            loss = resolve_criterion(criterion)(outputs, masks)
        elif loss_fn == "lovasz_softmax":
            loss = ops.lovasz_softmax(ops.softmax_channels(outputs), masks.long(), classes="present", per_image=False,
                                      ignore=ignore_label)
        elif loss_fn == "lovasz_hinge":
            loss = ops.lovasz_hinge(outputs, masks.long(), per_image=True, ignore=ignore_label)      # two planes: z1 - z0 in the kernel
        elif loss_fn == "cross_entropy":
            loss = ops.cross_entropy(outputs, masks.long(), -100 if ignore_label is None else int(ignore_label))
        else:
            raise ValueError(f"loss_fn {loss_fn!r}: 'cross_entropy', 'lovasz_softmax' or 'lovasz_hinge'")
        if extra_loss is not None:
            extra = extra_loss(outputs_x, images)
            if torch.is_tensor(extra) and extra.is_cuda and extra.dim() == 0 and loss.dim() == 0 and extra.dtype == loss.dtype:
                loss = ops.add_scalars(loss, extra)      # a launch of the library (visible to a launch plan)
            else:
                loss = loss + extra
    with ops.prof_range("train_step/backward"):
        optimizer.zero_grad()
        loss.backward(_one(loss.device) if (loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda) else None)
    with ops.prof_range("train_step/optimizer"):
        optimizer.step()
    return loss.detach()


def train_step_mean_teacher(model, ema, optimizer, images, masks, criterion=None, *, tau=0.9, mode="ignore", weight_by_conf=False):
    """One mean-teacher iteration: the EMA teacher (``ema.FlatEMA`` attached to ``optimizer``) corrects the batch's noisy labels,
    then the ordinary ``train_step`` runs on the corrected masks; returns its loss tensor.

    The teacher's eval-mode forward runs eagerly under ``no_grad``; ``ops.teacher_targets(teacher logits, masks clamped to
    {0, 1}, tau, mode)`` makes the labels - ``mode="ignore"`` (default) writes -100 where the teacher is confident and
    disagrees, which survives ``train_step``'s clamp and is the cross entropy's default ignore value; ``"replace"`` writes the
    teacher's class.  ``tau``: a number or a one-element float32 device tensor (a schedule).  ``weight_by_conf``: the teacher's
    confidence becomes the pixel weight of ``criterion``, which must then be a ``wnn.CrossEntropyLoss``
    (``criterion.set_pixel_weight(conf)``).  The student's step is the same call as without a teacher, so from its third
    occurrence it replays its launch plan - the corrected masks are plan inputs - and the EMA launches are part of that plan."""
    if ema is None or getattr(optimizer, "ema", None) is not ema or ema.model is not model:
        raise ValueError("train_step_mean_teacher: ema must be the FlatEMA attached to this optimizer for this model")
    if weight_by_conf and not isinstance(criterion, wnn.CrossEntropyLoss):
        raise ValueError("train_step_mean_teacher: weight_by_conf needs criterion=wnn.CrossEntropyLoss(...) (set_pixel_weight)")
    with torch.no_grad():
        logits = ema.teacher(images)["out"]
    labels = ops.clamp_max_labels(masks.long(), 1)
    if weight_by_conf:
        labels, conf = ops.teacher_targets(logits, labels, tau, mode, conf=True)
        criterion.set_pixel_weight(conf)
    else:
        labels = ops.teacher_targets(logits, labels, tau, mode)
    return train_step(model, optimizer, images, labels, criterion=criterion)


def train_step_consistency(model, ema, optimizer, images, masks, rows, criterion=None, *, consistency, photometric=True):
    """One view-consistency iteration: the EMA teacher (``ema.FlatEMA`` attached to ``optimizer``) predicts on ``images`` as they
    are, the student trains on an augmented VIEW of them, and ``consistency`` (a ``wnn.ConsistencyLoss``) adds the cost of the
    student disagreeing with the teacher's prediction warped onto that view; returns the loss tensor of ``train_step``.

    ``rows`` (B,8) float32 on the device: the view's parameter rows, ``Augment.draw(B, hw, hw)`` uploaded once per epoch as the
    loaders do - the map from the view's pixels to the pixels of ``images``, and so also the map from the student's grid to
    the teacher's.  Steps: (1) the teacher's eval-mode forward on ``images`` under ``no_grad`` (eager); (2) the view:
    ``ops.warp_scores(images, rows, photometric=photometric)`` and ``ops.warp_labels(masks, rows)`` - pixels the view takes from
    outside the image carry the label -100, which the cross entropy ignores, and are "not inside" for the consistency term;
    (3) ``consistency.set_teacher(teacher_logits, rows)``; (4) ``train_step(model, optimizer, view, labels,
    extra_loss=consistency, criterion=criterion)``.  The student's step is the same call every time, so from its third
    occurrence it replays one launch plan - view and labels are copied into the plan's inputs, the teacher buffer keeps its
    address - and ``consistency.set_lam`` ramps the weight without a new one.  The teacher's forward, the two warps, the
    ``masks.long()`` conversion and ``set_teacher``'s copies are issued eagerly on every call, in front of the plan."""
    if ema is None or getattr(optimizer, "ema", None) is not ema or ema.model is not model:
        raise ValueError("train_step_consistency: ema must be the FlatEMA attached to this optimizer for this model")
    if not isinstance(consistency, wnn.ConsistencyLoss):
        raise ValueError("train_step_consistency: consistency must be a wnn.ConsistencyLoss")
    with torch.no_grad():
        logits = ema.teacher(images)["out"]
        if tuple(logits.shape[-2:]) != tuple(images.shape[-2:]):
            raise ValueError(f"train_step_consistency: the teacher's logits {tuple(logits.shape[-2:])} are not at the images' size "
                             f"{tuple(images.shape[-2:])}: the view's rows would not map onto them")
        view = ops.warp_scores(images, rows, photometric=photometric)
        labels = ops.warp_labels(masks.long(), rows)
    consistency.set_teacher(logits, rows)
    return train_step(model, optimizer, view, labels, extra_loss=consistency, criterion=criterion)


def train_step_mixed(model, ema, optimizer, images, masks, mix, params, criterion=None, *, tau=0.9, weight_by_conf=False,
                     consistency=None):
    """One iteration on a MIXED batch - CutMix, ClassMix or copy-paste (``augment.Mix``), the strong perturbation of the
    teacher / student recipes (CutMix-Seg, ClassMix, DACS, UniMatch); returns the loss tensor of ``train_step``.

    ``mix``: an ``augment.Mix``; ``params``: this step's slice of its ``epoch_params`` (``Mix.step_params(params, i)``: partner,
    boxes, seeds on the device).  Steps:
    (1) the labels.  With ``ema`` (the ``ema.FlatEMA`` attached to ``optimizer``): the teacher's eval-mode forward on ``images``
        under ``no_grad``, then ``ops.teacher_targets(teacher logits, masks clamped to {0, 1}, tau, mode="replace",
        conf=weight_by_conf)``.  With ``ema=None``: ``masks`` as they are - plain CutMix or copy-paste on pseudo masks.
    (2) "classmix" / "copy_paste": ``ops.mix_class_select`` on those labels (``ema=None``: clamped to {0, 1}, as ``train_step``
        will see them), over the teacher's channel count of classes (2 without a teacher).
    (3) ONE ``ops.mix_batch`` over the images, the labels, the teacher's confidence as ``pixel_weight`` (``weight_by_conf``) and
        the teacher's logits as ``scores`` (``consistency``).
    (4) ``weight_by_conf``: ``criterion.set_pixel_weight(mixed confidence)`` - ``criterion`` must be a ``wnn.CrossEntropyLoss``, as
        for ``train_step_mean_teacher``.  ``consistency`` (a ``wnn.ConsistencyLoss``): ``consistency.set_teacher(mixed teacher
        logits)`` and it becomes the ``extra_loss`` - the mixed-teacher target of French et al.  Both need ``ema``.
    (5) ``train_step(model, optimizer, mixed images, mixed labels, ...)``: the same call every time, so from its third
        occurrence it replays one launch plan.  The teacher's forward and the mixing launches are issued eagerly on every
        call, in front of the plan, like the warps of ``train_step_consistency``.
    An item whose partner is -1 is unmixed: with every partner -1 the step equals ``train_step_mean_teacher(mode="replace")``
    (``ema=None``: ``train_step``) bit for bit."""
    if not isinstance(mix, Mix):
        raise ValueError("train_step_mixed: mix must be an augment.Mix")
    if ema is not None and (getattr(optimizer, "ema", None) is not ema or ema.model is not model):
        raise ValueError("train_step_mixed: ema must be the FlatEMA attached to this optimizer for this model (or None)")
    if ema is None and (weight_by_conf or consistency is not None):
        raise ValueError("train_step_mixed: weight_by_conf and consistency need the teacher (ema)")
    if weight_by_conf and not isinstance(criterion, wnn.CrossEntropyLoss):
        raise ValueError("train_step_mixed: weight_by_conf needs criterion=wnn.CrossEntropyLoss(...) (set_pixel_weight)")
    if consistency is not None and not isinstance(consistency, wnn.ConsistencyLoss):
        raise ValueError("train_step_mixed: consistency must be a wnn.ConsistencyLoss")
    labels, logits, conf, class_labels = masks.long(), None, None, None
    if ema is not None:
        with torch.no_grad():
            logits = ema.teacher(images)["out"]
        labels = ops.clamp_max_labels(labels, 1)
        if weight_by_conf:
            labels, conf = ops.teacher_targets(logits, labels, tau, "replace", conf=True)
        else:
            labels = ops.teacher_targets(logits, labels, tau, "replace")
    elif mix.kind != "cutmix":
        class_labels = ops.clamp_max_labels(labels, 1)
    mixed = mix.apply(images, labels, params, class_labels=class_labels, num_classes=2 if logits is None else int(logits.shape[1]),
                      pixel_weight=conf,
                      scores=logits if consistency is not None else None)
    if weight_by_conf:
        criterion.set_pixel_weight(mixed.pixel_weight)
    if consistency is not None:
        consistency.set_teacher(mixed.scores)
        return train_step(model, optimizer, mixed.images, mixed.labels, extra_loss=consistency, criterion=criterion)
    return train_step(model, optimizer, mixed.images, mixed.labels, criterion=criterion)


def make_optimizer(model, lr=1e-4, early_step=None, *, kind="adam", **optimizer_kwargs):
    """torch.optim.Adam(model.parameters(), lr) semantics on one flat buffer.  ``kind``: 'adam' (optim.FlatAdam), 'adamw'
    (optim.FlatAdamW) or 'sgd' (optim.FlatSGD); ``optimizer_kwargs`` go to that class (weight_decay, momentum, nesterov,
    max_grad_norm, skip_nonfinite, no_decay, betas, eps ...) - the standard DeepLabV3 recipe is ``kind="sgd", momentum=0.9,
    weight_decay=1e-4`` with ``optim.PolyLR``.  Single process: one Adam launch per step,
    then the re-layout of every convolution weight on the side stream.  Under ``dp.GradBucketReducer`` the buffer is
    stepped in segments (optim.FlatAdam.enable_early_step): each segment's Adam launch and the re-layout of its
    convolution weights follow its gradient all-reduce.  ``early_step=True`` (or WSDL_EARLY_STEP=1) uses the segments
    in a single process too."""
    params = [p for p in model.parameters() if p.requires_grad]
    classes = {"adam": FlatAdam, "adamw": FlatAdamW, "sgd": FlatSGD}
    if kind not in classes:
        raise ValueError(f"kind {kind!r}: 'adam', 'adamw' or 'sgd'")
    opt = classes[kind](params, lr=lr, **optimizer_kwargs)
    convs = [m for m in model.modules() if isinstance(m, wnn.Conv2d) and m.weight.requires_grad and m.weight.is_cuda]
    if convs:
        index = {id(p): i for i, p in enumerate(params)}
        by_param = {index[id(m.weight)]: m for m in convs}

        def relayout(k, param_indices, use_events, adam_event=None):
            if k == 0:
                adam_event = None        # the first layers' layouts gate the next forward: not behind the other segments' queue
            seg_convs = [by_param[i] for i in param_indices if i in by_param]
            # runs before step() bumps the parameter epoch; in eager mode into the spare buffers (this step's remaining
            # input-gradient kernels still read the current ones), inside a captured graph in place
            return ops.prefetch_weight_layouts(seg_convs, use_events=use_events, epoch_ahead=1, pingpong=use_events,
                                               after=adam_event)

        opt.post_step_hook = lambda: ops.prefetch_weight_layouts(convs)     # after the single-launch step
        if early_step is None:
            early_step = {"0": False, "1": True, "2": "tail"}[os.environ.get("WSDL_EARLY_STEP", "0")]
        if early_step == "tail":
            # two segments: [the stem | everything else].  "Everything else" is stepped while the stem's backward (max-pool,
            # BatchNorm over the 67 MB map, the 7x7 weight gradient: 0.3 ms of small launches) still runs
            stem = params[0].numel() + sum(p.numel() for p in params[1:3])
            opt.enable_early_step(relayout, first=(stem + 63) // 64 * 64, growth=1 << 20, cap=1 << 40)
        else:
            opt.enable_early_step(relayout)
        opt.early_step = bool(early_step)
        if opt.early_step:
            opt.register_announce_hooks()
    return opt


MULTISCALE_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


@torch.no_grad()
def predict_multiscale(model, images, scales=MULTISCALE_SCALES, flip=True, *, multiple=32, activation="softmax", scores=False,
                       min_conf=0.0, ignore_index=255):
    """Multi-scale + flip inference, the protocol DeepLab-family results are reported with: images (B,3,H,W) on the device ->
    int64 labels (B,H,W), or ``(labels, scores)`` with ``scores=True`` (float32 (B,C,H,W), the fused map).

    In eval mode (the model's mode is restored afterwards) and without gradients: per scale ONE ``ops.scale_flip`` to
    ``ops.multiscale_sizes(H, W, scales, multiple)`` and ONE network pass over ``[plain; mirrored]`` that stops at the stride-8
    logits (``model.head_logits``; a model without it gives ``model(x)["out"]``), then ONE ``ops.multiscale_fuse`` launch to
    H x W: ``activation`` per member ('softmax': probabilities are averaged, 'none': logits), the mean over scales and mirror
    images, the arg-max (``ignore_index`` where the fused maximum is below ``min_conf``).  No full-size map per scale exists.

    With the default split arithmetic of the convolutions an image's logits depend on which images share its device batch (one
    scale per tensor - the effect the README notes for coalesced CAMs); the mirrored half therefore shares a batch with the plain
    half, and a prediction is reproducible for the same batch, not across batch compositions."""
    if not torch.is_tensor(images) or images.dim() != 4:
        raise ValueError("predict_multiscale: images must be (B,3,H,W)")
    H, W = int(images.shape[-2]), int(images.shape[-1])
    sizes = ops.multiscale_sizes(H, W, scales, multiple)
    was_training = model.training
    model.eval()
    try:
        head = getattr(model, "head_logits", None)
        sources = []
        for size in sizes:
            x = ops.scale_flip(images, size, flip)
            sources.append(head(x) if head is not None else model(x)["out"])
        res = ops.multiscale_fuse(sources, (H, W), mirrored=bool(flip), activation=activation, scores=bool(scores), labels=True,
                                  min_conf=min_conf, ignore_index=ignore_index)
    finally:
        if was_training:
            model.train()
    return (res[1], res[0]) if scores else res


@torch.no_grad()
def evaluate_model(model, loader, device="cuda", binarize="notebook", *, scales=None, flip=False):
    """argmax -> nearest resize to the ground truth's size -> IoU / pixel accuracy, averaged over the loader's images
    (one image - the first of each batch - per batch, as the reference).  Ground truth from the Oxford-IIIT Pet trimap:
      binarize="notebook": ``tm[tm == 2] = 1; tm = 1 - tm``      (AlternatingDirectionCutLoss.py:639-682, the script
                           that actually runs - SURVEY.md section 0);
      binarize="modular" : ``tm = (tm == 1)``                    (SegmentationModel.py:126-159).
    ``scales`` / ``flip`` (keyword-only; the default ``None`` / ``False`` is the single-scale body above, launch for launch):
    the prediction is ``predict_multiscale(model, x, scales or (1.0,), flip)`` - softmax probabilities averaged over the scales
    and the mirror image - with the same image selection, ground-truth rule and nearest resize.  (Its note on device batches
    applies: here every batch is one image and its mirror image.)"""
    model.eval()
    multi = scales is not None or bool(flip)
    ious, accs = [], []
    for img, (_label, true_mask) in loader:
        x = img[0].to(device).unsqueeze(0)
        tm = true_mask[0].to(device).clone()
        if binarize == "notebook":
            tm[tm == 2] = 1
            tm = 1 - tm
        elif binarize == "modular":
            tm = (tm == 1).long()
        else:
            raise ValueError(binarize)
        if multi:
            pred = predict_multiscale(model, x, (1.0,) if scales is None else scales, flip)[0]
        else:
            out = model(x)["out"]
            pred = out.squeeze(0).argmax(dim=0)
        if pred.shape != tm.shape:
            # F.interpolate(mode='nearest'): source index = floor(dst * in / out)
            idx_h = (torch.arange(tm.shape[-2], device=device) * pred.shape[0] // tm.shape[-2])
            idx_w = (torch.arange(tm.shape[-1], device=device) * pred.shape[1] // tm.shape[-1])
            pred = pred[idx_h][:, idx_w]
        iou, acc = compute_iou_and_acc(pred, tm)
        ious.append(iou)
        accs.append(acc)
    return sum(ious) / len(ious), sum(accs) / len(accs)


@torch.no_grad()
def evaluate_calibration(model, loader, device="cuda", binarize="notebook", bins=15):
    """Whether the model's confidence means what it says, over the images ``evaluate_model`` scores - the first of each batch, the
    same ground-truth rule (``binarize``), the logits nearest-resized to the ground truth's size by its index rule: the softmax
    maximum of every pixel is binned over ``bins`` uniform bins of [0, 1] by whether the arg-max is right
    (``ops.confidence_histogram``, one launch per image); the tables are added on the device and copied to the host once, after
    the loop.  Returns a dict: ``ece`` - the expected calibration error; ``accuracy`` / ``confidence`` / ``count`` - the
    reliability curve, one entry per bin (NaN where a bin is empty); ``tau_0.9`` / ``tau_0.95`` - the smallest confidence edge at
    and above which 90 % / 95 % of the pixels are right (``ops.tau_for_precision``; None if there is none): what ``tau`` of
    ``teacher_targets`` would have to be for that precision; ``counts`` / ``sums`` - the pooled tables."""
    model.eval()
    total = None
    for img, (_label, true_mask) in loader:
        x = img[0].to(device).unsqueeze(0)
        tm = true_mask[0].to(device).clone()
        if binarize == "notebook":
            tm[tm == 2] = 1
            tm = 1 - tm
        elif binarize == "modular":
            tm = (tm == 1).long()
        else:
            raise ValueError(binarize)
        tm = tm.reshape(tm.shape[-2:]).long()
        out = model(x)["out"]
        if out.shape[-2:] != tm.shape:
            idx_h = (torch.arange(tm.shape[-2], device=device) * out.shape[-2] // tm.shape[-2])
            idx_w = (torch.arange(tm.shape[-1], device=device) * out.shape[-1] // tm.shape[-1])
            out = out[:, :, idx_h][:, :, :, idx_w]
        tables = torch.stack(ops.confidence_histogram(out.contiguous(), tm[None].contiguous(), bins=bins, per_image=False))
        total = tables if total is None else total + tables
    if total is None:
        raise ValueError("evaluate_calibration: the loader is empty")
    counts, sums = total.cpu().numpy()                                     # the one copy to the host
    ece, acc, conf, cnt = ops.ece_from_counts(counts, sums)
    edges = ops.uniform_edges(0.0, 1.0, bins)
    return {"ece": ece, "accuracy": acc, "confidence": conf, "count": cnt, "tau_0.9": ops.tau_for_precision(counts, edges, 0.9),
            "tau_0.95": ops.tau_for_precision(counts, edges, 0.95), "counts": counts, "sums": sums}


@torch.no_grad()
def evaluate_boundary_iou(model, loader, device="cuda", binarize="notebook", ratio=0.02):
    """Mean Boundary IoU (Cheng et al., CVPR 2021; ``ops.boundary_iou``) of the foreground over the images ``evaluate_model``
    scores - the first of each batch, the same ground-truth rule (``binarize``) and the same nearest resize of the argmax -
    with the band width ``ops.boundary_width`` of each ground truth's size and ``ratio``.  Region IoU on 224 x 224 pets is
    dominated by the interior; this one moves when a refinement step moves the contour.  The counts of every image land
    in a row of their own on the device; one copy after the loop brings them to the host."""
    model.eval()
    rows = torch.zeros(len(loader), 2, dtype=torch.int64, device=device)
    n = 0
    for img, (_label, true_mask) in loader:
        x = img[0].to(device).unsqueeze(0)
        tm = true_mask[0].to(device).clone()
        if binarize == "notebook":
            tm[tm == 2] = 1
            tm = 1 - tm
        elif binarize == "modular":
            tm = (tm == 1).long()
        else:
            raise ValueError(binarize)
        pred = model(x)["out"].squeeze(0).argmax(dim=0)
        if pred.shape != tm.shape:
            idx_h = (torch.arange(tm.shape[-2], device=device) * pred.shape[0] // tm.shape[-2])
            idx_w = (torch.arange(tm.shape[-1], device=device) * pred.shape[1] // tm.shape[-1])
            pred = pred[idx_h][:, idx_w]
        ops.boundary_iou_counts(pred[None], tm.long()[None], ops.boundary_width(tm.shape[-2], tm.shape[-1], ratio), out=rows[n:n + 1])
        n += 1
    return ops.boundary_iou_from_counts(rows[:n].cpu().numpy())


@torch.no_grad()
def evaluate_surface_distances(model, loader, device="cuda", binarize="notebook", percentile=95.0):
    """Mean Hausdorff distance, its ``percentile`` (HD95) and the average symmetric surface distance of the foreground, in
    pixels, over the images ``evaluate_boundary_iou`` scores - the first of each batch, the same ground-truth rule
    (``binarize``) and the same nearest resize of the argmax.  Region IoU and Boundary IoU are overlaps; these say how many
    pixels a contour is off.  ``ops.surface_distance_stats`` per image; the statistics of every image land in a row of their
    own on the device and one copy after the loop brings them to the host.  Returns ``(means, n_defined)``: a dict with
    ``"hd"``, ``"hd95"`` and ``"assd"`` over the ``n_defined`` images where both the prediction and the ground truth have a
    foreground pixel (``nan`` when there is none) - the conventions of ``ops.surface_distances_from_stats``."""
    ops.check_percentile(percentile)
    model.eval()
    rows = torch.zeros(len(loader), 8, dtype=torch.float64, device=device)
    n = 0
    for img, (_label, true_mask) in loader:
        x = img[0].to(device).unsqueeze(0)
        tm = true_mask[0].to(device).clone()
        if binarize == "notebook":
            tm[tm == 2] = 1
            tm = 1 - tm
        elif binarize == "modular":
            tm = (tm == 1).long()
        else:
            raise ValueError(binarize)
        pred = model(x)["out"].squeeze(0).argmax(dim=0)
        if pred.shape != tm.shape:
            idx_h = (torch.arange(tm.shape[-2], device=device) * pred.shape[0] // tm.shape[-2])
            idx_w = (torch.arange(tm.shape[-1], device=device) * pred.shape[1] // tm.shape[-1])
            pred = pred[idx_h][:, idx_w]
        ops.surface_stats_rows(ops.surface_distance_stats(pred[None], tm.long()[None], percentile=percentile), out=rows[n:n + 1])
        n += 1
    _per, means, defined = ops.surface_distances_from_stats(ops.surface_stats_from_rows(rows[:n].cpu().numpy()))
    return means, defined


def train_segmentation_model(loss_fn, run_id, lr=1e-4, num_epochs=10, batch_size=4, val_split=0.2, *, out_root="/content",
                             device="cuda", val_loader=None, num_workers=0, seed=None, log=print, model=None,
                             optimizer_kind="adam", optimizer_kwargs=None, criterion=None, ema=None):
    """Reference ``train_segmentation_model(loss_fn, run_id, lr=1e-4, num_epochs=10, batch_size=4, val_split=0.2)``
    (TraditionalModel/SegmentationModel.py:59-122), same positional signature, returns ``(model, final_loss)``.

    Trains DeepLabV3-ResNet50 (``build_segmentation_model``) with Adam(lr) on the pseudo masks of run ``run_id`` -
    ``{out_root}/images_{run_id}`` / ``{out_root}/pseudo_masks_{run_id}``, what ``generate_pseudo_masks`` wrote - with
    ``loss_fn`` 'cross_entropy', 'lovasz_softmax' or 'lovasz_hinge'; batches of one image are skipped (:97-98), masks clamped to {0,1} (:100).

    Where the reference's text cannot run, the working notebook decides: the reference builds the
    pseudo-mask dataset (:73-77) and then trains on ``load_split_data()`` (:80-83), whose items are not (image, mask)
    pairs; AlternatingDirectionCutLoss.py:775-781 trains on ``PseudoSegmentationDataset`` - so does this.  ``val_split`` is
    accepted and, as in the reference (which never reads it), unused; the per-epoch validation of :118-119 runs when a
    ``val_loader`` of ``(img, (label, trimap))`` items is given (the reference takes it from the Oxford-IIIT Pet download,
    which needs the network).  Keyword-only extras: the directories' root (the reference hard-codes /content), the
    device, an existing model to continue from, ``optimizer_kind`` / ``optimizer_kwargs`` (``make_optimizer``'s ``kind`` and
    keyword arguments; the default is the reference's Adam(lr)), ``criterion`` (handed to ``train_step`` in place of
    ``loss_fn``'s loss, e.g. ``wnn.MinedCrossEntropyLoss(mode="trim", drop_frac=0.2)`` against the label noise of the pseudo
    masks; ``None``: the ``loss_fn`` loss as before), ``ema`` (a dict of ``ema.FlatEMA`` keywords, e.g. ``{"decay": 0.999}``: a
    teacher - a second ``build_segmentation_model`` - follows the weights by their moving average; it is validated beside
    the student, and the ``FlatEMA`` is left as ``model.ema``, its ``teacher`` the network to predict and refine with;
    ``None``: no launch is added)."""
    from torch.utils.data import DataLoader
    from .SegmentationDataset import PseudoSegmentationDataset
    if loss_fn not in ("cross_entropy", "lovasz_softmax", "lovasz_hinge"):
        raise ValueError(f"loss_fn {loss_fn!r}: 'cross_entropy', 'lovasz_softmax' or 'lovasz_hinge'")
    import os as _os
    image_dir = _os.path.join(out_root, f"images_{run_id}")
    mask_dir = _os.path.join(out_root, f"pseudo_masks_{run_id}")
    full_dataset = PseudoSegmentationDataset(img_dir=image_dir, mask_dir=mask_dir, transform=True)
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    train_loader = DataLoader(full_dataset, batch_size=batch_size, shuffle=True, num_workers=num_workers, generator=gen)
    if model is None:
        model = build_segmentation_model(num_classes=2)
    model = model.to(device)
    optimizer = make_optimizer(model, lr=lr, kind=optimizer_kind, **(optimizer_kwargs or {}))
    averaged = None
    if ema is not None:
        from ..ema import FlatEMA
        num_classes = model.classifier[-1].out_channels if isinstance(model, SegmentationModel) else 2
        teacher = build_segmentation_model(num_classes=num_classes, aux_loss=getattr(model, "aux_classifier", None) is not None)
        averaged = FlatEMA(optimizer, model, teacher.to(device), **dict(ema))
        model.ema = averaged                            # (a plain object: not a sub-module, not part of the state dict)
    final_loss = 0.0
    for epoch in range(num_epochs):
        model.train()
        total = torch.zeros((), device=device)
        for images, masks in train_loader:
            if images.size(0) == 1:
                continue
            total += train_step(model, optimizer, images.to(device), masks.to(device), loss_fn=loss_fn, criterion=criterion)
        final_loss = total.item()                       # one host read per epoch (the reference: one per step)
        if log:
            log(f"[Run {run_id}] Epoch {epoch + 1}/{num_epochs}, Loss: {final_loss:.4f}")
        if val_loader is not None:
            avg_iou, avg_acc = evaluate_model(model, val_loader, device=device, binarize="modular")
            if log:
                log(f"[Run {run_id}] Validation IoU: {avg_iou:.4f}, Accuracy: {avg_acc:.4f}")
            if averaged is not None:
                t_iou, t_acc = evaluate_model(averaged.teacher, val_loader, device=device, binarize="modular")
                if log:
                    log(f"[Run {run_id}] EMA teacher validation IoU: {t_iou:.4f}, Accuracy: {t_acc:.4f}")
    return model, final_loss
