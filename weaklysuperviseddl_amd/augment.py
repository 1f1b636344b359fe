"""Joint image / label augmentation for the device-resident loaders (host side of csrc/augment.hip).

The reference has no augmentation; this is the standard segmentation recipe its training loops lack: random scale,
rotation and horizontal flip applied to image and label together, plus a light photometric jitter of the image.  An
``Augment`` only DRAWS parameters - one row ``a00 a01 a02 a10 a11 a12 gain bias`` per item, the affine map from output to
source pixel coordinates and the photometric map ``gain * value + bias`` - and ``ops.augment_batch`` applies them in one
launch together with the loader's gather, its uint8 -> float table and its label mapping.

No host -> device copy happens per step: a loader draws the rows of a whole epoch when its iteration starts, uploads them
once and hands every batch its slice (``epoch_params``).

Fill modes.  ``fill="ignore"``: output pixels whose source point lies outside the image get ``pad_value`` and the label
``pad_label``.  The default -100 survives ``clamp_max_labels`` and is the default ``ignore_index`` of ``ops.cross_entropy``,
so cross entropy ignores the padding as it is; the Lovasz losses need ``train_step(..., ignore_label=-100)``.
``fill="reflect"``: the source is mirrored about its borders, every output pixel is valid and nothing needs ignoring - the
mode to use with the NCut and boundary terms, which would otherwise see an edge at the pad border.
"""
import math

import torch

IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)


def _pair(v, name):
    lo, hi = (float(v), float(v)) if isinstance(v, (int, float)) else (float(v[0]), float(v[1]))
    if not (0.0 < lo <= hi):
        raise ValueError(f"{name} {v!r}: 0 < low <= high")
    return lo, hi


class Augment:
    """``scale``      (low, high) magnification of the content, uniform: 0.5 shrinks it to half the output, 2 shows the
                   central half of the source;
    ``rotate``     largest angle in degrees: the angle is uniform in [-rotate, rotate];
    ``hflip``      probability of a horizontal flip;
    ``brightness`` the bias is uniform in [-brightness, brightness];
    ``contrast``   the gain is uniform in [1 - contrast, 1 + contrast];
    ``fill``, ``pad_value``, ``pad_label``: see the module text; ``out_size``: (out_h, out_w) of the batches, None = the
    source's size (a different size resamples the whole source onto the output before the augmentation applies).

    Draw order (``sample``): for n items, n values each of scale, angle, flip, bias, gain - in this order, as float64
    ``torch.rand(n, generator=generator)``; a component that cannot vary (a one-point scale range, ``rotate`` /
    ``brightness`` / ``contrast`` of 0, ``hflip`` of 0 or 1) draws nothing, so the identity leaves the generator alone."""

    def __init__(self, scale=(1.0, 1.0), rotate=0.0, hflip=0.0, brightness=0.0, contrast=0.0, fill="ignore", pad_value=0.0,
                 pad_label=-100, out_size=None):
        self.scale = _pair(scale, "scale")
        self.rotate, self.hflip = float(rotate), float(hflip)
        self.brightness, self.contrast = float(brightness), float(contrast)
        if self.rotate < 0 or not (0.0 <= self.hflip <= 1.0) or self.brightness < 0 or self.contrast < 0:
            raise ValueError("Augment: rotate, brightness and contrast are non-negative, hflip is a probability")
        if fill not in ("ignore", "reflect"):
            raise ValueError(f"fill {fill!r}: 'ignore' or 'reflect'")
        self.fill, self.pad_value, self.pad_label = fill, float(pad_value), int(pad_label)
        self.out_size = None if out_size is None else (int(out_size[0]), int(out_size[1]))

    @classmethod
    def identity(cls, **kwargs):
        """The augmentation that changes nothing: every row it draws is ``1 0 0 0 1 0 1 0``."""
        return cls(**kwargs)

    def sample(self, n, generator=None):
        """The raw draws of n items as float64 tensors: scale, angle (degrees), flip (0 / 1), bias, gain."""
        n = int(n)

        def uniform(lo, hi):
            if lo == hi:
                return torch.full((n,), lo, dtype=torch.float64)
            return lo + (hi - lo) * torch.rand(n, generator=generator, dtype=torch.float64)

        scale = uniform(*self.scale)
        angle = uniform(-self.rotate, self.rotate)
        if 0.0 < self.hflip < 1.0:
            flip = (torch.rand(n, generator=generator, dtype=torch.float64) < self.hflip).to(torch.float64)
        else:
            flip = torch.full((n,), self.hflip, dtype=torch.float64)
        bias = uniform(-self.brightness, self.brightness)
        gain = uniform(1.0 - self.contrast, 1.0 + self.contrast)
        return {"scale": scale, "angle": angle, "flip": flip, "bias": bias, "gain": gain}

    @staticmethod
    def compose(sample, src_hw, out_hw):
        """(n,8) float32 rows of the draws: the map from output to source coordinates, composed in float64 about the image
        centres and cast once.  With d = (u - out_w / 2, v - out_h / 2) the source point is
        ``diag(W / out_w, H / out_h) . F . R(angle) . d / scale + (W / 2, H / 2)``, F = diag(-1, 1) for a flip,
        R(t) = [[cos t, -sin t], [sin t, cos t]]."""
        H, W = (float(v) for v in src_hw)
        Ho, Wo = (float(v) for v in out_hw)
        s = sample["scale"].to(torch.float64)
        t = torch.deg2rad(sample["angle"].to(torch.float64))
        f = 1.0 - 2.0 * sample["flip"].to(torch.float64)
        cos, sin = torch.cos(t), torch.sin(t)
        rx, ry = W / Wo, H / Ho
        a00, a01 = rx * f * cos / s, -(rx * f * sin / s)
        a10, a11 = ry * sin / s, ry * cos / s
        a02 = W / 2 - (a00 * (Wo / 2) + a01 * (Ho / 2))
        a12 = H / 2 - (a10 * (Wo / 2) + a11 * (Ho / 2))
        rows = torch.stack([a00, a01, a02, a10, a11, a12, sample["gain"].to(torch.float64),
                            sample["bias"].to(torch.float64)], dim=1)
        return (rows + 0.0).to(torch.float32)           # (+ 0.0: no negative zeros in the rows)

    def draw(self, n, src_hw, out_hw, generator=None):
        """(n,8) float32 CPU tensor: the parameter rows of n items (``sample`` then ``compose``)."""
        return self.compose(self.sample(n, generator), src_hw, out_hw)

    def out_hw(self, src_hw):
        return tuple(int(v) for v in (src_hw if self.out_size is None else self.out_size))

    def epoch_params(self, n, src_hw, device, generator=None):
        """The rows of a whole epoch of n items, drawn now and uploaded once; a loader slices them per batch."""
        return self.draw(n, src_hw, self.out_hw(src_hw), generator).to(device)

    def apply(self, images, labels, idx, params, *, lut=None, label_lut=None):
        """``ops.augment_batch`` with this object's fill, padding and output size."""
        from . import ops
        return ops.augment_batch(images, labels, idx, params, self.out_hw(images.shape[-2:]), lut=lut, label_lut=label_lut,
                                 fill=self.fill, pad_value=self.pad_value, pad_label=self.pad_label)


def affine_row(angle_deg, src_hw, out_hw=None, scale=1.0, flip=False, gain=1.0, bias=0.0):
    """One parameter row for fixed values (tests, tools): ``Augment.compose`` of a single draw."""
    one = lambda v: torch.tensor([float(v)], dtype=torch.float64)          # noqa: E731
    sample = {"scale": one(scale), "angle": one(angle_deg), "flip": one(1.0 if flip else 0.0), "bias": one(bias),
              "gain": one(gain)}
    return Augment.compose(sample, src_hw, src_hw if out_hw is None else out_hw)[0]


def relative_rows(student_rows, teacher_rows=None):
    """(n,8) float32 rows of ``T^-1 o S``: the map from a STUDENT view's output pixel to the pixel of the TEACHER's view, for two
    views of the same source drawn as ``student_rows`` (S) and ``teacher_rows`` (T), each mapping its output to source pixel
    coordinates.  What ``ops.consistency_loss(student_logits, teacher, rows)`` and ``ops.warp_scores(teacher, rows)`` take to
    bring a teacher's prediction onto the student's grid.  ``teacher_rows=None``: the teacher sees the source as it is, the
    result is the affine part of ``student_rows``.  Composed in float64 with tensor operations on whatever device the rows
    live on and cast once; the gain / bias columns are ``1 0`` (a prediction is not re-coloured).  A singular teacher row gives
    a non-finite row, which the kernels treat as "nowhere inside"."""
    s = torch.as_tensor(student_rows)
    if s.dim() != 2 or s.shape[1] != 8:
        raise ValueError(f"relative_rows: student_rows must be (n,8), got {tuple(s.shape)}")
    s = s.to(torch.float64)
    if teacher_rows is None:
        a = s[:, :6]
    else:
        t = torch.as_tensor(teacher_rows)
        if tuple(t.shape) != tuple(s.shape) or t.device != s.device:
            raise ValueError(f"relative_rows: teacher_rows must be {tuple(s.shape)} on {s.device}, got {tuple(t.shape)} on {t.device}")
        t = t.to(torch.float64)
        t00, t01, t02, t10, t11, t12 = t[:, :6].unbind(1)
        det = t00 * t11 - t01 * t10
        i00, i01, i10, i11 = t11 / det, -(t01 / det), -(t10 / det), t00 / det           # T's linear part inverted
        s00, s01, s02, s10, s11, s12 = s[:, :6].unbind(1)
        dx, dy = s02 - t02, s12 - t12
        a = torch.stack([i00 * s00 + i01 * s10, i00 * s01 + i01 * s11, i00 * dx + i01 * dy,
                         i10 * s00 + i11 * s10, i10 * s01 + i11 * s11, i10 * dx + i11 * dy], dim=1)
    ones, zeros = torch.ones_like(a[:, :1]), torch.zeros_like(a[:, :1])
    return (torch.cat([a, ones, zeros], dim=1) + 0.0).to(torch.float32)


_MIX_KINDS = ("cutmix", "classmix", "copy_paste")


class Mix:
    """Batch mixing - CutMix, ClassMix, copy-paste - for teacher / student training.  Like ``Augment`` a ``Mix`` only DRAWS
    parameters; ``ops.mix_class_select`` and ``ops.mix_batch`` apply them on the device (``apply``).

    ``kind``     "cutmix": item b takes a box (the union of ``boxes`` boxes) from its partner;
                 "classmix": it takes the pixels of half of the classes present in the partner's label map, chosen on the device
                 from the item's seed;
                 "copy_paste": it takes the partner's pixels of class 1, the foreground (``candidates = (1,)``).
    ``prob``     probability that an item is mixed at all; an unmixed item has the partner -1.
    ``area``     (low, high) fraction of the image one box covers, uniform;
    ``aspect``   (low, high) width / height of a box, log-uniform;
    ``boxes``    R, boxes per item, 1..8;
    ``partner``  "roll": one shift s per batch, item b is mixed with item (b + s) mod B, s in [1, B - 1] - never itself;
                 "permute": a random permutation per batch (fixed points mix an item with itself, which changes nothing).

    Draw order (``draw``), everything for all ``n_batches`` at once and each component only if it can vary:
      1. partners - "roll" with B >= 3: ``torch.randint(1, B, (n_batches,))`` (B = 2 has the one shift 1, B = 1 the shift 0:
         nothing is drawn); "permute" with B >= 2: ``torch.randperm(B)`` once per batch;
      2. 0 < ``prob`` < 1: ``torch.rand(n_batches, B)`` float64, an item is mixed where the draw is below ``prob``;
      3. "cutmix" only, each as ``torch.rand(n_batches, B, R)`` float64: the area fraction (unless ``area`` is one point), the
         aspect (unless ``aspect`` is one point), the row position, the column position;
      4. "classmix" only: the seeds, ``torch.randint(0, 2**32, (n_batches, B, 2))`` joined to one int64 each.
    Whatever is not drawn is zeros: ``boxes`` of empty boxes, ``seeds`` of 0 (copy-paste's single candidate is taken whenever
    it is present: no seed can change that)."""

    def __init__(self, kind="cutmix", prob=1.0, area=(0.25, 0.5), aspect=(0.5, 2.0), boxes=1, partner="roll"):
        if kind not in _MIX_KINDS:
            raise ValueError(f"Mix: kind {kind!r}: 'cutmix', 'classmix' or 'copy_paste'")
        if partner not in ("roll", "permute"):
            raise ValueError(f"Mix: partner {partner!r}: 'roll' or 'permute'")
        self.kind, self.partner, self.prob = kind, partner, float(prob)
        if not 0.0 <= self.prob <= 1.0:
            raise ValueError(f"Mix: prob {prob!r} is a probability")
        self.area, self.aspect = _pair(area, "area"), _pair(aspect, "aspect")
        if self.area[1] > 1.0:
            raise ValueError(f"Mix: area {area!r}: fractions of the image, at most 1")
        if isinstance(boxes, bool) or not isinstance(boxes, int) or not 1 <= boxes <= 8:
            raise ValueError(f"Mix: boxes {boxes!r}: an int in 1..8")
        self.boxes = boxes
        self.candidates = (1,) if kind == "copy_paste" else None          # the class list of ops.mix_class_select

    def draw(self, n_batches, B, hw, generator=None):
        """The parameters of ``n_batches`` batches of B items with planes of ``hw`` = (H, W), as CPU tensors: ``{"partner": int32
        (n_batches,B), "boxes": int32 (n_batches,B,R,4), "seeds": int64 (n_batches,B)}``.  Boxes are rows ``(y0, x0, y1, x1)``,
        half-open: with f the area fraction and r the aspect, ``h = sqrt(f H W / r)``, ``w = sqrt(f H W r)`` in float64, each
        rounded once and clamped to [1, H] / [1, W]; the position is uniform over the places where the box fits, so every box
        lies inside the image with at least one pixel."""
        n, B = int(n_batches), int(B)
        H, W = (int(v) for v in hw)
        if n < 0 or B < 1 or H < 1 or W < 1:
            raise ValueError(f"Mix.draw: n_batches {n_batches!r}, B {B!r}, hw {hw!r}")
        R = self.boxes
        f64 = torch.float64
        item = torch.arange(B, dtype=torch.int64)
        if self.partner == "roll":
            if B >= 3:
                shift = torch.randint(1, B, (n,), generator=generator, dtype=torch.int64)
            else:
                shift = torch.full((n,), B - 1, dtype=torch.int64)
            partner = (item[None, :] + shift[:, None]) % B
        elif B >= 2:
            partner = torch.stack([torch.randperm(B, generator=generator) for _ in range(n)]) if n else torch.zeros(0, B, dtype=torch.int64)
        else:
            partner = torch.zeros(n, B, dtype=torch.int64)
        if 0.0 < self.prob < 1.0:
            mixed = torch.rand(n, B, generator=generator, dtype=f64) < self.prob
        else:
            mixed = torch.full((n, B), self.prob == 1.0)
        partner = torch.where(mixed, partner, torch.full_like(partner, -1)).to(torch.int32)

        boxes = torch.zeros(n, B, R, 4, dtype=torch.int32)
        if self.kind == "cutmix":
            def uniform(lo, hi):
                if lo == hi:
                    return torch.full((n, B, R), lo, dtype=f64)
                return lo + (hi - lo) * torch.rand(n, B, R, generator=generator, dtype=f64)
            frac = uniform(*self.area)
            aspect = torch.exp(uniform(math.log(self.aspect[0]), math.log(self.aspect[1])))
            uy = torch.rand(n, B, R, generator=generator, dtype=f64)
            ux = torch.rand(n, B, R, generator=generator, dtype=f64)
            h = torch.sqrt(frac * (H * W) / aspect).round().clamp(1, H).to(torch.int64)
            w = torch.sqrt(frac * (H * W) * aspect).round().clamp(1, W).to(torch.int64)
            y0 = torch.minimum((uy * (H - h + 1).to(f64)).floor().to(torch.int64), H - h)
            x0 = torch.minimum((ux * (W - w + 1).to(f64)).floor().to(torch.int64), W - w)
            boxes = torch.stack([y0, x0, y0 + h, x0 + w], dim=-1).to(torch.int32)
        seeds = torch.zeros(n, B, dtype=torch.int64)
        if self.kind == "classmix":
            words = torch.randint(0, 2 ** 32, (n, B, 2), generator=generator, dtype=torch.int64)
            seeds = (words[..., 0] - 2 ** 31) * 2 ** 32 + words[..., 1]
        return {"partner": partner, "boxes": boxes, "seeds": seeds}

    def epoch_params(self, n_batches, B, hw, device, generator=None):
        """The parameters of a whole epoch, drawn now and uploaded once; step i takes ``step_params(params, i)``."""
        return {k: v.to(device) for k, v in self.draw(n_batches, B, hw, generator).items()}

    @staticmethod
    def step_params(params, i):
        """Slice ``[i]`` of every tensor of ``epoch_params``: views, no copy and no host -> device traffic."""
        return {k: v[i] for k, v in params.items()}

    def apply(self, images, labels, params_i, *, class_labels=None, num_classes=2, pixel_weight=None, scores=None, want_mask=False,
              want_count=False, out=None):
        """Mix one batch with the parameters of its step (``step_params``) -> ``ops.MixResult``.  "cutmix": one
        ``ops.mix_batch(kind="box")``; "classmix" / "copy_paste": ``ops.mix_class_select`` on ``class_labels`` (default: ``labels``)
        with ``num_classes`` and this object's ``candidates``, then ``ops.mix_batch(kind="class")``."""
        from . import ops
        kw = dict(pixel_weight=pixel_weight, scores=scores, want_mask=want_mask, want_count=want_count, out=out)
        if self.kind == "cutmix":
            return ops.mix_batch(images, labels, params_i["partner"], kind="box", boxes=params_i["boxes"], **kw)
        cls = labels if class_labels is None else class_labels
        sel, _ = ops.mix_class_select(cls, num_classes, params_i["seeds"], candidates=self.candidates)
        return ops.mix_batch(images, labels, params_i["partner"], kind="class", class_labels=cls, sel=sel, **kw)


__all__ = ["Augment", "IDENTITY_ROW", "Mix", "affine_row", "relative_rows"]
