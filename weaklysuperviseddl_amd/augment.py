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


__all__ = ["Augment", "IDENTITY_ROW", "affine_row", "relative_rows"]
