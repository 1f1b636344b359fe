"""FlatAdam - torch.optim.Adam semantics (defaults betas=(0.9,0.999), eps=1e-8, no weight decay;
reference TraditionalModel/SegmentationModel.py:91) as ONE kernel launch over flat buffers.  Beyond the reference: weight
decay (L2 or decoupled: ``FlatAdamW``), SGD with momentum (``FlatSGD``), clipping by the global gradient norm, skipping of steps
whose gradient is not finite, parameters without decay, and ``PolyLR`` - all of it read from device memory by the kernels of
csrc/flat_optim.hip, so a launch plan of the step survives a schedule; with those arguments at their defaults the launches are
the ones below, unchanged.  An ``ema.FlatEMA`` registers itself as ``optimizer.ema``: its average of the parameters is one
more launch right behind every step launch, on that launch's range (``_launch_ema``); without one nothing is added.

Parameters are re-homed into one contiguous fp32 buffer (``p.data`` become views) and so are their
gradients (``p.grad`` views of one flat buffer), which is also what the data-parallel gradient
all-reduce buckets (``dp.GradBucketReducer``) operate on: 39.6 M parameters = 158.5 MB per replica.

Segment steps (``enable_early_step``; used under data parallelism, opt-in for a single process - measured 0.4 %
slower there: six Adam launches instead of one, nothing left to hide).  The update is element-wise, so the flat buffer
can be stepped in pieces.
Backward fills it from the last layer to the first; the buffer is cut (on parameter boundaries) into segments that grow
geometrically from the FIRST layers - 1 MB, 5 MB, 25 MB, then at most 48 MB each - and a segment's Adam launch, the
amax of its convolution weights and their re-layout for the next step are enqueued on the side stream as soon as
its last expected gradient has been announced, behind the weight-gradient kernels that produce it.  What is left when
``step()`` is called is the small first segment: the stem and layer1.  Which parameters are "expected" is learnt from the previous step (the aux head of the
segmentation model never receives a gradient); a gradient that turns up for a parameter whose segment has already been
stepped raises.  The same segments are the data-parallel reducer's buckets: the all-reduce exposed at the end of
backward is the 1 MB one.
"""
import contextlib
import torch

from . import ops

_ALIGN = 64   # floats; keeps every parameter 256-byte aligned inside the flat buffer
import os as _os
# what FlatAdam does when the sentinel fires: "auto" (the default since round 6: switch the range guards on for the steps that
# follow - the reference's fp32 has no range floor, so the default must not keep computing below it) | "warn" (say so, change
# nothing) | "off"
RANGE_GUARD_DEFAULT = "auto"
RANGE_GUARD = [_os.environ.get("WSDL_RANGE_GUARD", RANGE_GUARD_DEFAULT)]
RANGE_GUARD_ACTIVE = [False]                                  # "auto" has switched the guards on in this process
RANGE_SENTINEL = [_os.environ.get("WSDL_RANGE_SENTINEL", "1") != "0"]      # FlatAdam.step() checks the step's tensors for regions below the fp16x2 arithmetic's safe range


def _is_norm_module(m):
    from . import nn as wnn
    import torch.nn as tnn
    return isinstance(m, (wnn.BatchNorm2d, wnn.GroupNorm, tnn.modules.batchnorm._BatchNorm, tnn.GroupNorm, tnn.LayerNorm))


def no_decay_norm_and_bias(model):
    """The parameters weight decay usually leaves alone: everything a normalisation layer owns (BatchNorm scale and shift)
    and every bias.  Returns a list to pass as ``no_decay=``."""
    out, seen = [], set()
    for m in model.modules():
        for name, p in m.named_parameters(recurse=False):
            if id(p) not in seen and (_is_norm_module(m) or name == "bias" or name.endswith("_bias")):
                seen.add(id(p))
                out.append(p)
    return out


def build_decay_blocks(offsets, numels, total, no_decay_flags):
    """The weight-decay table of the step kernel: one uint8 per ``_ALIGN`` floats of a flat buffer of ``total`` floats, 1 where
    decay applies.  ``offsets`` / ``numels``: where each parameter starts (a multiple of ``_ALIGN``) and how long it is;
    ``no_decay_flags[i]`` true: parameter i's blocks are 0.  The padding behind a parameter follows the parameter."""
    if total % _ALIGN:
        raise ValueError(f"build_decay_blocks: total {total} is not a multiple of {_ALIGN}")
    table = torch.ones(total // _ALIGN, dtype=torch.uint8)
    for off, n, flag in zip(offsets, numels, no_decay_flags):
        if off % _ALIGN or off + n > total:
            raise ValueError(f"build_decay_blocks: parameter at {off} (+{n}) does not sit on a {_ALIGN}-float boundary inside {total}")
        if flag:
            table[off // _ALIGN:(off + n + _ALIGN - 1) // _ALIGN] = 0
    return table


def _no_decay_flags(params, no_decay):
    if no_decay is None:
        return [False] * len(params)
    if callable(no_decay):
        return [bool(no_decay(p)) for p in params]
    ids = {id(p) for p in no_decay}
    return [id(p) in ids for p in params]


class FlatAdam:
    """Adam on one flat buffer.  With the keyword arguments at their defaults this is torch.optim.Adam's default step through
    ``ops.adam_step_flat`` - exactly the launches it always issued.  ``weight_decay`` (L2 as torch.optim.Adam, or
    ``decoupled=True``: torch.optim.AdamW), ``max_grad_norm`` (torch.nn.utils.clip_grad_norm_ on the whole gradient),
    ``skip_nonfinite`` (a step whose gradient norm is inf / NaN changes nothing) and ``no_decay`` (a predicate or a
    collection of parameters without weight decay) go through ``ops.grad_norm`` / ``ops.flat_step`` (csrc/flat_optim.hip).
    ``max_grad_norm`` / ``skip_nonfinite`` with ``weight_decay=0`` run the Adam + L2 instantiation with wd = 0: the same
    algorithm, but not the default launch bit for bit (``g += 0 * p`` makes the gradient of a parameter that is already inf
    a NaN, where the default kernel never multiplies the parameter)."""
    _early_step = False
    ema = None                      # an ``ema.FlatEMA`` registers itself here: its launches follow every step launch

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, *, weight_decay=0.0, decoupled=False,
                 max_grad_norm=None, skip_nonfinite=False, no_decay=None):
        self._check_args(weight_decay, 0.0, False, max_grad_norm)
        self.betas, self.eps = betas, eps
        self.decoupled = bool(decoupled)
        self.momentum, self.nesterov = 0.0, False
        self._setup(params, lr, grad_scale, weight_decay, max_grad_norm, skip_nonfinite, no_decay, ("exp_avg", "exp_avg_sq"))

    @staticmethod
    def _check_args(weight_decay, momentum, nesterov, max_grad_norm):
        # (host only: no device is touched before the arguments are known to be good)
        if weight_decay < 0:
            raise ValueError(f"weight_decay {weight_decay}: must be >= 0")
        if momentum < 0:
            raise ValueError(f"momentum {momentum}: must be >= 0")
        if nesterov and momentum <= 0:
            raise ValueError("nesterov momentum needs momentum > 0 (and zero dampening)")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm {max_grad_norm}: must be > 0 (None: no clipping)")

    def _setup(self, params, lr, grad_scale, weight_decay, max_grad_norm, skip_nonfinite, no_decay, state_names):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError(f"{type(self).__name__}: empty parameter list")
        dev = self.params[0].device
        self.lr, self.grad_scale = lr, grad_scale
        self.weight_decay, self.max_grad_norm, self.skip_nonfinite = weight_decay, max_grad_norm, bool(skip_nonfinite)
        self.step_count = 0             # calls of step(); the kernels read step_dev, which a skipped step does not advance
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32) if dev.type == "cuda" else None   # device twin
        # lr, beta1, beta2, eps, grad_scale as the Adam kernel reads them, then weight_decay, momentum, nesterov, max_norm,
        # skip_nonfinite for the flat step (device floats: a schedule or a reducer changing one of them changes memory, not a
        # launch - a recorded launch plan of the step stays valid); sync_hyper() keeps them current
        self.hyper_dev = torch.zeros(ops.FLAT_HYPER, device=dev, dtype=torch.float32) if dev.type == "cuda" else None
        # total_norm, clip_coef, apply, skipped_steps - written by the norm's finalize launch, read by the step kernel
        self.stats_dev = torch.tensor([0., 1., 1., 0.], device=dev, dtype=torch.float32) if dev.type == "cuda" else None
        self._norm_partials = (torch.zeros(ops.grad_norm_partials(), device=dev, dtype=torch.float64)
                               if dev.type == "cuda" else None)     # scratch of the norm's first launch
        self._hyper_host = None
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = n
        self.flat_param = torch.zeros(n, device=dev, dtype=torch.float32)
        self.flat_grad = torch.zeros(n, device=dev, dtype=torch.float32)
        for name in ("exp_avg", "exp_avg_sq"):          # (FlatSGD: exp_avg is the momentum buffer, None without momentum)
            setattr(self, name, torch.zeros(n, device=dev, dtype=torch.float32) if name in state_names else None)
        flags = _no_decay_flags(self.params, no_decay)
        self.decay_blocks = None        # None: weight decay everywhere
        if any(flags):
            self.decay_blocks = build_decay_blocks(self.offsets, [p.numel() for p in self.params], n, flags).to(dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                view = self.flat_param[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
        self.segments = None           # early segment steps: [(lo, hi)] on parameter boundaries, None = one launch in step()
        self.pre_step_hook = None      # e.g. wait for the gradient all-reduce
        self.post_step_hook = None     # e.g. prefetch next step's weight layouts on the side stream
        # direct gradient delivery: the HIP backward kernels write each parameter's gradient straight into
        # its flat_grad slice (ops._sink_of); `_fresh` = not yet written since zero_grad (first write overwrites)
        self._fresh = {id(p): True for p in self.params}
        self.grad_ready_hooks = []     # callables(param): fired when a parameter's gradient has been written
        for p in self.params:
            p._wsdl_grad_sink = self

    # ---------------------------------------------------------------------------------- early segment steps
    def enable_early_step(self, segment_hook=None, first=1 << 18, growth=5, cap=12_000_000):
        """Cut the flat buffer into segments and step each as soon as its gradients are complete (module docstring).
        ``segment_hook(k, param_indices, use_events, adam_event)`` runs right after segment k's Adam launch: the place to
        re-lay-out that segment's convolution weights (behind ``adam_event``, on a stream of its own)."""
        if not self.flat_param.is_cuda:
            return self
        bounds, target = [0], first
        for off in self.offsets[1:]:
            if off - bounds[-1] >= target:
                bounds.append(off)
                target = min(target * growth, cap)
        if len(bounds) > 1 and self.numel - bounds[-1] < first:
            bounds.pop()                               # no crumb at the end
        bounds.append(self.numel)
        self.segments = [(bounds[i], bounds[i + 1]) for i in range(len(bounds) - 1)]
        self.seg_of = []
        for off in self.offsets:
            self.seg_of.append(max(k for k, (lo, _hi) in enumerate(self.segments) if lo <= off))
        self.seg_params = [[i for i, k in enumerate(self.seg_of) if k == kk] for kk in range(len(self.segments))]
        self.segment_hook = segment_hook
        self._early_step = False        # True: step segments as backward completes them (False: one launch in step(),
                                        # unless a data-parallel reducer drives the segments - external_trigger)
        self.external_trigger = False   # True: someone else (the DP reducer) decides when a segment is complete
        self.capture_mode = False       # inside hipGraph capture: no cross-replay events
        self._index = {id(p): i for i, p in enumerate(self.params)}
        self._expected = None           # parameter indices that fired in the previous step
        self._fired = set()
        self._stepped = [False] * len(self.segments)
        self._remaining = None
        self._accumulating = False
        self._adam_event = None
        self._prep_done = [None] * len(self.segments)     # per segment: event behind its last re-layout
        self._seg_events = [None] * len(self.segments)    # per segment: event behind its Adam launch
        self._hooked = False
        return self

    def register_announce_hooks(self):
        """Gradient announcements (needed only when segments are stepped before ``step()``: 364 Python hook calls per step
        of the segmentation model cost the host ~2.5 ms of the 16 it needs to enqueue a step)."""
        if self.segments is None or self._hooked:
            return
        self._hooked = True
        for i, p in enumerate(self.params):
            p.register_post_accumulate_grad_hook(lambda q, i=i: self._announce(i))
        self.grad_ready_hooks.append(lambda p: self._announce(self._index[id(p)]))

    @contextlib.contextmanager
    def accumulate(self):
        """Backward passes inside the context only accumulate gradients (no early segment step)."""
        self._accumulating = True
        try:
            yield
        finally:
            self._accumulating = False

    def _announce(self, i):
        if i in self._fired:
            return
        self._fired.add(i)
        k = self.seg_of[i]
        if self._stepped[k]:
            raise RuntimeError(
                f"FlatAdam: a gradient for parameter {i} {tuple(self.params[i].shape)} arrived after its segment had been "
                "stepped (a parameter that received no gradient in the previous step, or a second backward before "
                "step()).  Wrap extra backward passes in optimizer.accumulate() or set optimizer.early_step = False.")
        if self.external_trigger or not self.early_step or self.capture_mode or self._accumulating or self._expected is None:
            return
        if i in self._expected:
            self._remaining[k] -= 1
        # segments leave in backward order, a segment only once every later one has left
        for kk in range(len(self.segments) - 1, -1, -1):
            if self._stepped[kk]:
                continue
            if self._remaining[kk] > 0:
                break
            self.step_segment(kk)

    def step_segment(self, k, after=None):
        """Adam on segment k, enqueued on the side stream behind the main stream's work so far (BatchNorm / bias
        gradients, the input-gradient kernels that still read this segment's weight layouts) and behind ``after``
        (a collective's work handle)."""
        self._refuse_early_norm()
        dev = self.flat_param.device
        lo, hi = self.segments[k]
        side = ops.side_stream(dev)
        ops.stream_wait(side, ops.raw_stream(dev))
        if not self.capture_mode and self._prep_done[k] is not None:
            self._prep_done[k].wait(side)              # last step's re-layouts of THIS segment read the parameters overwritten now
        ev = None
        with torch.cuda.stream(side):
            if after is not None:
                after.wait()
            if not any(self._stepped):
                self.step_count += 1
                ops.add_int(self.step_dev, 1)
            self._launch(lo, hi)
            if self.ema is not None:
                # the average of this segment right behind its step; the buffers once, behind the last segment
                self._launch_ema(lo, hi, last=sum(self._stepped) == len(self.segments) - 1)
            if not self.capture_mode:
                ev = self._seg_events[k]               # one event per segment, re-recorded step after step
                if ev is None:
                    ev = self._seg_events[k] = ops.Event()
                self._adam_event = ev
                ev.record(side)
        self._stepped[k] = True
        if self.segment_hook is not None:
            self._prep_done[k] = self.segment_hook(k, self.seg_params[k], not self.capture_mode, ev)

    def _finish_segments(self):
        dev = self.flat_param.device
        for k in range(len(self.segments) - 1, -1, -1):
            if not self._stepped[k]:
                self.step_segment(k)
        if self.capture_mode or self._adam_event is None:
            ops.stream_wait(ops.raw_stream(dev), ops.side_stream(dev))
        else:
            self._adam_event.wait(ops.raw_stream(dev))   # the parameters, not the re-layouts behind them on the side stream
        self._expected = set(self._fired)
        self._fired = set()
        self._stepped = [False] * len(self.segments)
        self._remaining = [sum(1 for i in idx if i in self._expected) for idx in self.seg_params]
        self._backward_pending = False

    # ---------------------------------------------------------------------------------- which launches a step issues
    def algo(self):
        """None: the default Adam step (``ops.adam_step_flat``); else the ``ops.FLAT_*`` algorithm of ``ops.flat_step``."""
        if self.weight_decay == 0 and not self.needs_norm():
            return None
        return ops.FLAT_ADAMW if self.decoupled else ops.FLAT_ADAM_L2

    def needs_norm(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def launch_key(self):
        """What of the optimiser's settings selects LAUNCHES (not values in device memory): part of a launch plan's key."""
        key = (self.algo(), self.needs_norm(), self.decay_blocks is not None)
        return key if self.ema is None else key + (self.ema.launch_key(),)

    @property
    def early_step(self):
        return self._early_step

    @early_step.setter
    def early_step(self, value):
        if value and self.needs_norm():
            raise RuntimeError(self._EARLY_NORM)
        self._early_step = value

    _EARLY_NORM = ("max_grad_norm / skip_nonfinite need the norm of the WHOLE gradient before any parameter is stepped: segments "
                   "cannot be stepped while backward still runs.  Set optimizer.early_step = False (under a data-parallel reducer "
                   "the buffer is then stepped once, behind the last all-reduce).")

    def _refuse_early_norm(self):
        if self.needs_norm():
            raise RuntimeError(self._EARLY_NORM)

    def _hyper_values(self):
        return (float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.grad_scale),
                float(self.weight_decay), float(self.momentum), float(bool(self.nesterov)),
                float(self.max_grad_norm or 0.0), float(bool(self.skip_nonfinite)))

    def state_tensors(self):
        """Every device tensor of the optimiser a step changes in place (a launch plan's verification compares and restores
        them): parameters, state buffers, the device step number, the norm / skip statistics."""
        own = [t for t in (self.flat_param, self.exp_avg, self.exp_avg_sq, self.step_dev, self.stats_dev) if t is not None]
        return own if self.ema is None else own + self.ema.state_tensors()     # (the average, the teacher's buffers, start_dev)

    def _grad_norm_launches(self):
        ops.grad_norm(self.flat_grad, self.hyper_dev, self.step_dev, self.stats_dev, self._norm_partials)

    def grad_norm(self):
        """Norm of the (grad_scale-averaged) gradient as a device scalar, no synchronisation: with clipping / skipping on, what
        the last step measured before it clipped; otherwise measured now from the gradient buffer."""
        if not self.flat_grad.is_cuda:
            raise ops.WsdlError("grad_norm: gradients are not on the device; there is no CPU fallback")
        if not self.needs_norm():
            self.sync_hyper()
            self._grad_norm_launches()
        return self.stats_dev[0]

    def skipped_steps(self):
        """How many steps ``skip_nonfinite`` has dropped, as a device scalar (float), no synchronisation."""
        if self.stats_dev is None:
            raise ops.WsdlError("skipped_steps: the optimiser is not on the device")
        return self.stats_dev[3]

    def _launch_ema(self, lo, hi, last):
        """The attached EMA's launches behind the step launch on [lo, hi) (``last``: no step launch follows in this step)."""
        self.ema.launch(lo, hi)
        if last:
            self.ema.launch_buffers()

    def _launch(self, lo, hi):
        """The step launch on [lo, hi) of the flat buffers (the whole buffer, or one segment: ``lo`` on a parameter boundary)."""
        algo = self.algo()
        cut = (lambda t: None if t is None else t[lo:hi]) if (lo, hi) != (0, self.numel) else (lambda t: t)
        if algo is None:
            ops.adam_step_flat(cut(self.flat_param), cut(self.flat_grad), cut(self.exp_avg), cut(self.exp_avg_sq), self.lr,
                               self.betas[0], self.betas[1], self.eps, self.step_count, self.grad_scale,
                               step_dev=self.step_dev, hyper_dev=self.hyper_dev)
            return
        table = self.decay_blocks
        if table is not None and (lo, hi) != (0, self.numel):
            table = table[lo // _ALIGN:(hi + _ALIGN - 1) // _ALIGN]
        ops.flat_step(algo, cut(self.flat_param), cut(self.flat_grad), cut(self.exp_avg), cut(self.exp_avg_sq), self.hyper_dev,
                      self.step_dev, self.stats_dev if self.needs_norm() else None, table)

    def sync_hyper(self):
        """Copy (lr, beta1, beta2, eps, grad_scale, weight_decay, momentum, nesterov, max_norm, skip_nonfinite) to the device when
        one of them changed since the last call.

        Never inside a stream capture: the copy is a pageable host-to-device transfer (illegal in a hipGraph capture, and a
        captured copy would freeze the values anyway).  ``GraphedTrainStep`` calls this BEFORE it captures and before every
        replay, so the captured Adam node reads current values from ``hyper_dev``; a change that turns up while a capture is
        running is an error, not something to skip silently."""
        cur = self._hyper_values()
        if self.ema is not None:
            self.ema.sync_hyper()
        if self.hyper_dev is not None and cur != self._hyper_host:
            if self.hyper_dev.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FlatAdam.sync_hyper: a value of hyper_dev (lr, betas, eps, grad_scale, weight_decay, momentum, "
                                   "nesterov, max_grad_norm, skip_nonfinite) changed inside a stream capture; change "
                                   "them between steps (GraphedTrainStep copies them to the device before each replay)")
            self.hyper_dev.copy_(torch.tensor(cur, dtype=torch.float32))
            self._hyper_host = cur

    def take_fresh(self, p):
        f = self._fresh.get(id(p), False)
        self._fresh[id(p)] = False
        return f

    def grad_ready(self, p):
        self._dirty = True              # the side stream may be writing flat_grad: zero_grad must join before its memset
        for h in self.grad_ready_hooks:
            h(p)

    def zero_grad(self, set_to_none=False):
        self.sync_hyper()               # (segments may be stepped from backward hooks, before step() is reached)
        if self.flat_grad.is_cuda and getattr(self, "_dirty", True):
            ops.join_side_stream(self.flat_grad.device)      # a backward without a step may still be writing
        if self.flat_grad.is_cuda:
            ops.memset_zero(self.flat_grad)         # a launch of the library: part of a recorded plan
        else:
            self.flat_grad.zero_()
        for k in self._fresh:
            self._fresh[k] = True
        for p, off in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = self.flat_grad[off:off + p.numel()].view_as(p)

    def tail_ms(self):
        """Mean main-stream time of the optimiser tail over the steps taken while ``time_tail`` was set: from the entry of
        ``step()`` (backward's last main-stream kernel is enqueued) to its exit (the parameters are written: the next forward
        may start).  Single process: the join with the weight-gradient stream + Adam.  Under ``GradBucketReducer``: also what
        the main stream waits for the gradient collectives - the EXPOSED communication is this figure minus the
        single-process one."""
        pairs, self._tail_events = getattr(self, "_tail_events", []), []
        if not pairs:
            return None
        torch.cuda.synchronize(self.flat_param.device)
        return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)

    def step(self):
        if getattr(self, "time_tail", False) and self.flat_param.is_cuda and not self.capture_mode:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return self._step()
            finally:
                e1.record()
                self.__dict__.setdefault("_tail_events", []).append((e0, e1))
        return self._step()

    def range_poll(self):
        """Host side of the range sentinel (no synchronisation: the check kernels of the step before write pinned host memory):
        warn once when a tensor of the last step spanned more than the fp16x2 arithmetic's safe range - and, with
        ``WSDL_RANGE_GUARD=auto``, switch both range guards on for the steps that follow (weight layouts and launch plans
        re-form by themselves: ops.set_option bumps their epochs).  Called by the eager step and after every plan replay."""
        if getattr(self, "_range_warned", False) or getattr(self, "_range_hold", False) or RANGE_GUARD[0] == "off" or \
                not (RANGE_SENTINEL[0] and ops.CONV_ARITH[0] == 1):
            return
        st = ops.range_status(self.flat_param.device)
        if not st["exceeded"]:
            return
        self._range_warned = True
        import warnings
        what = (f"weaklysuperviseddl_amd: {st['pairs_over_limit']} activation / gradient tensors of the last step span more than "
                f"2^{st['limit_log2']} between their largest and their smallest region (worst 2^{st['worst_log2']:.0f}): the default "
                "convolution arithmetic (fp16x2, one scale per tensor) computes the small regions to fewer than 13 bits there - ")
        if RANGE_GUARD[0] == "auto":
            ops.set_option("conv_arith", 2)
            ops.set_option("wgrad_chan_scale", 1)
            RANGE_GUARD_ACTIVE[0] = True
            warnings.warn(what + "WSDL_RANGE_GUARD=auto: the range guards are on from the next step (conv_arith = 2, wgrad_chan_scale = 1; "
                          "about 10 % slower)")
        else:
            warnings.warn(what + "select the range guards: ops.set_option('conv_arith', 2) (forward / input gradient) and "
                          "ops.set_option('wgrad_chan_scale', 1) (weight gradient), or WSDL_RANGE_GUARD=auto")

    def _sentinel(self):
        """Range sentinel of the fp16x2 arithmetic (every exit of a step, the segmented / data-parallel one too): what the
        PREVIOUS step's tensors spanned, then this step's check - behind the join with the side stream, whose pools it reads."""
        if self.flat_param.is_cuda and RANGE_SENTINEL[0] and ops.CONV_ARITH[0] == 1 and not self.capture_mode_on():
            self.range_poll()
            ops.range_check(self.flat_param.device)

    def capture_mode_on(self):
        return bool(getattr(self, "capture_mode", False))

    def _step(self):
        self.sync_hyper()
        if self.pre_step_hook is not None:
            # (the data-parallel reducer's wait(): collectives' work handles, control-plane exchange - host work that a launch
            # plan repeats live at this place)
            ops.host_section(self.pre_step_hook)
        if self.segments is not None:
            if self.external_trigger or self.early_step or any(self._stepped):
                self._finish_segments()         # (the segment hook has re-laid-out the weights)
                ops.bump_param_epoch()
                self._dirty = False             # the main stream waits for the Adam launches, which follow every gradient
                self._sentinel()
                return
            self._fired = set()                 # one launch over the whole buffer, below
        if self.flat_param.is_cuda:
            ops.join_side_stream(self.flat_param.device)     # weight gradients are produced on the side stream
        self.step_count += 1
        ops.bump_param_epoch()          # parameters change behind torch's version counters
        if self.flat_param.is_cuda:
            # the kernel reads the step number from the device: a captured (hipGraph) step replays correctly
            ops.add_int(self.step_dev, 1)
            if self.needs_norm():
                # the whole gradient is in flat_grad here (hook run, side stream joined): norm, clip coefficient and the
                # skip decision stay on the device, the step launch reads them
                self._grad_norm_launches()
            self._launch(0, self.numel)
            if self.ema is not None:
                self._launch_ema(0, self.numel, last=True)
        else:
            raise ops.WsdlError("FlatAdam.step: parameters are not on the device; there is no CPU fallback")
        self._dirty = False                     # (joined above)
        self._sentinel()
        if self.post_step_hook is not None:
            self.post_step_hook()


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW: ``FlatAdam`` with decoupled weight decay, default 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, *, weight_decay=1e-2, decoupled=True,
                 max_grad_norm=None, skip_nonfinite=False, no_decay=None):
        super().__init__(params, lr, betas, eps, grad_scale, weight_decay=weight_decay, decoupled=decoupled,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, no_decay=no_decay)


class FlatSGD(FlatAdam):
    """torch.optim.SGD (dampening 0) on the flat buffers: ``g += wd p; buf = mu buf + g; g = nesterov ? g + mu buf : buf;
    p -= lr g`` - the zero-initialised buffer reproduces torch's first step.  A subclass of ``FlatAdam`` for everything
    that is not the arithmetic: the flat layout, gradient sinks, segments, hooks, ``sync_hyper``, launch plans.  ``exp_avg``
    is the momentum buffer (None when constructed without momentum), there is no second buffer."""
    def __init__(self, params, lr=1e-3, momentum=0.0, nesterov=False, weight_decay=0.0, *, grad_scale=1.0, max_grad_norm=None,
                 skip_nonfinite=False, no_decay=None):
        self._check_args(weight_decay, momentum, nesterov, max_grad_norm)
        self.betas, self.eps = (0.0, 0.0), 0.0          # (unused by the SGD kernel; the slots of hyper_dev stay)
        self.decoupled = False
        self.momentum, self.nesterov = momentum, bool(nesterov)
        self._setup(params, lr, grad_scale, weight_decay, max_grad_norm, skip_nonfinite, no_decay,
                    ("exp_avg",) if momentum > 0 else ())

    def algo(self):
        return ops.FLAT_SGD

    def _hyper_values(self):
        self._check_args(self.weight_decay, self.momentum, self.nesterov, self.max_grad_norm)
        if self.momentum > 0 and self.exp_avg is None:
            raise ValueError("FlatSGD: momentum was switched on after construction without momentum: there is no buffer for it")
        return super()._hyper_values()


class PolyLR:
    """torch.optim.lr_scheduler.PolynomialLR with a linear warm-up and a floor, for the flat optimisers: ``step()`` sets
    ``optimizer.lr`` on the host, ``sync_hyper()`` carries it to the device before the next step - no kernel, and a recorded
    launch plan is kept.  After ``t`` calls of ``step()``:
      t <  warmup_steps: lr = base_lr (t + 1) / (warmup_steps + 1)
      t >= warmup_steps: lr = min_lr + (base_lr - min_lr) (1 - min(t - warmup_steps, T) / T) ** power,  T = total_steps - warmup_steps
    (``warmup_steps = 0, min_lr = 0``: PolynomialLR(total_iters=total_steps, power) in closed form)."""

    def __init__(self, optimizer, total_steps, power=0.9, warmup_steps=0, min_lr=0.0):
        if total_steps <= 0 or not 0 <= warmup_steps < total_steps:
            raise ValueError("PolyLR: total_steps > 0 and 0 <= warmup_steps < total_steps")
        if min_lr < 0 or power <= 0:
            raise ValueError("PolyLR: min_lr >= 0 and power > 0")
        self.optimizer, self.total_steps, self.power = optimizer, int(total_steps), float(power)
        self.warmup_steps, self.min_lr = int(warmup_steps), float(min_lr)
        self.base_lr = float(optimizer.lr)
        self.last_step = 0
        optimizer.lr = self.lr_at(0)

    def lr_at(self, t):
        if t < self.warmup_steps:
            return self.base_lr * (t + 1) / (self.warmup_steps + 1)
        T = self.total_steps - self.warmup_steps
        left = 1.0 - min(t - self.warmup_steps, T) / T
        return self.min_lr + (self.base_lr - self.min_lr) * left ** self.power

    def step(self):
        self.last_step += 1
        self.optimizer.lr = self.lr_at(self.last_step)
        return self.optimizer.lr

    def get_last_lr(self):
        return [self.optimizer.lr]
