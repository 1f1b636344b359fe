"""FlatEMA - the exponential moving average of the weights over training (the "mean teacher" copy, Tarvainen & Valpola 2017) for
the flat optimisers, as launches of the library ordered behind the step launch.

The parameters live in ``FlatAdam.flat_param`` and are rewritten by kernels behind torch's version counters; a training step is
replayed as a launch plan that sees only launches of the C ABI; ``skip_nonfinite`` decides on the device whether a step
happened; early segment steps update the buffer piecewise.  So the average is ``ops.flat_ema`` on a second flat buffer
(``ema_param``, the student's offsets) right behind every step launch on that launch's range, plus one ``ops.ema_table`` launch
for the float buffers (BatchNorm running statistics).  Both read the optimiser's own device step number and skip word: a skipped
step updates nothing and does not advance the warm-up.  The teacher is a second instance of the architecture whose parameters
are views into ``ema_param``; its eval-mode caches are keyed on ``ops.PARAM_EPOCH`` / ``ops.STATS_EPOCH``, which every step -
eager or replayed - bumps.

Not built: the average fused into the step kernels (it would save the re-read of ``p``, 4 of 40 bytes per element), hipGraph
capture of these launches (``GraphedTrainStep`` refuses an optimiser with an EMA), fp16 / bf16 teacher storage, SWA-style equal
averaging and BatchNorm re-estimation.
"""
import torch

from . import ops

_BUFFER_MODES = ("ema", "copy")


def check_decay(decay, name="FlatEMA"):
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay < 1.0:
        raise ValueError(f"{name}: decay {decay!r} must be a number in [0, 1)")
    return float(decay)


def warmup_decay(decay, k):
    """The decay of update number ``k`` (0-based) with warm-up on, as the kernels form it: ``min(decay, (1 + k) / (10 + k))`` with
    both sides rounded to float32 (``ops.flat_ema``)."""
    f32 = torch.tensor([float(decay), (1.0 + k) / (10.0 + k)], dtype=torch.float32)
    return float(f32.min())


def _match(model, teacher):
    """Student and teacher must agree by key, shape and dtype (host only)."""
    if teacher is model:
        raise ValueError("FlatEMA: the teacher must be a second instance of the architecture, not the student itself")
    out = []
    for what, s_named, t_named in (("parameter", dict(model.named_parameters()), dict(teacher.named_parameters())),
                                   ("buffer", dict(model.named_buffers()), dict(teacher.named_buffers()))):
        missing = sorted(set(s_named) ^ set(t_named))
        if missing:
            raise ValueError(f"FlatEMA: student and teacher do not have the same {what}s: {missing[:4]}"
                             + (" ..." if len(missing) > 4 else ""))
        for k, s in s_named.items():
            t = t_named[k]
            if tuple(s.shape) != tuple(t.shape) or s.dtype != t.dtype:
                raise ValueError(f"FlatEMA: {what} {k}: student {tuple(s.shape)} {s.dtype}, teacher {tuple(t.shape)} {t.dtype}")
            if t is s:
                raise ValueError(f"FlatEMA: {what} {k} is shared between student and teacher")
        out.append((s_named, t_named))
    return out


class FlatEMA:
    """``FlatEMA(optimizer, model, teacher)``: after every applied step of ``optimizer`` (``FlatAdam`` / ``FlatAdamW`` /
    ``FlatSGD``; with clipping, skipping, early segment steps, launch plans), ``teacher <- d teacher + (1 - d) model`` with
    ``d = decay``, or with ``warmup`` ``min(decay, (1 + k) / (10 + k))`` for the k-th update (0-based; the ratio rounded to float32).  The arithmetic is
    ``ops.flat_ema``'s: in double, rounded once.

    ``teacher``: a second instance of the same architecture, built by the caller (``build_segmentation_model()``) on the
    optimiser's device - matched by key, shape and dtype; any mismatch raises before the device is touched.  Every teacher
    parameter whose student parameter the optimiser owns becomes a view into ``ema_param`` (a device copy of ``flat_param``),
    ``requires_grad=False``; frozen student parameters are copied once.  Float buffers are averaged (``buffers="ema"``) or
    copied (``"copy"``: the teacher keeps the student's statistics) after every applied step; integer buffers
    (``num_batches_tracked``) are copied in ``state_dict()`` / ``sync_counters()`` only.  The teacher is put into ``eval()``.

    Constructing it registers it as ``optimizer.ema``; the step's launch plan then holds its launches and verifies
    ``ema_param``, the teacher's buffers and ``start_dev`` with the rest of the state.  Under a data-parallel reducer every
    rank holds identical parameters and so identical averages; the student's BatchNorm statistics are per rank, so
    ``buffers="ema"`` averages per-rank statistics and ``buffers="copy"`` gives per-rank statistics, as the student has.

    A NaN or inf parameter propagates into the average: ``skip_nonfinite=True`` on the optimiser is the guard."""

    def __init__(self, optimizer, model, teacher, decay=0.999, warmup=True, buffers="ema"):
        self.decay = check_decay(decay)
        if buffers not in _BUFFER_MODES:
            raise ValueError(f"FlatEMA: buffers {buffers!r}: 'ema' or 'copy'")
        if getattr(optimizer, "ema", None) is not None:
            raise ValueError("FlatEMA: the optimiser already has an EMA attached")
        (s_params, t_params), (s_bufs, t_bufs) = _match(model, teacher)
        index = {id(p): i for i, p in enumerate(optimizer.params)}
        if not any(id(p) in index for p in s_params.values()):
            raise ValueError("FlatEMA: the optimiser owns none of the model's parameters")
        dev = optimizer.flat_param.device
        if dev.type != "cuda" or optimizer.step_dev is None:
            raise ops.WsdlError("FlatEMA: the optimiser is not on the device; there is no CPU fallback")
        for k, t in list(t_params.items()) + list(t_bufs.items()):
            if t.device != dev:
                raise ops.WsdlError(f"FlatEMA: teacher tensor {k} is on {t.device}, the optimiser on {dev}")
        self.opt, self.model, self.teacher = optimizer, model, teacher
        self.warmup, self.buffers = bool(warmup), buffers
        self.ema_param = optimizer.flat_param.clone()
        self._frozen, self._float_bufs, self._int_bufs = [], [], []
        with torch.no_grad():
            for k, sp in s_params.items():
                tp = t_params[k]
                i = index.get(id(sp))
                if i is None:
                    self._frozen.append((tp, sp))
                    tp.data.copy_(sp.data)
                else:
                    off = optimizer.offsets[i]
                    tp.data = self.ema_param[off:off + sp.numel()].view_as(sp)
                tp.requires_grad_(False)
                tp.grad = None
            for k, sb in s_bufs.items():
                tb = t_bufs[k]
                if sb.dtype == torch.float32 and sb.numel() > 0:
                    if not tb.is_contiguous() or not sb.is_contiguous():
                        raise ops.WsdlError(f"FlatEMA: buffer {k} is not dense")
                    self._float_bufs.append((tb, sb))
                else:
                    self._int_bufs.append((k, tb))
                tb.copy_(sb)
        self._table = ops.ema_table_entries(self._float_bufs, dev) if self._float_bufs else None
        self.hyper_dev = torch.zeros(2, device=dev, dtype=torch.float32)
        self._hyper_host = None
        self.start_dev = optimizer.step_dev.clone()
        self.sync_hyper()
        teacher.eval()
        ops.bump_param_epoch()
        ops.bump_stats_epoch()
        optimizer.ema = self

    # ---------------------------------------------------------------------------------- what the optimiser calls
    def launch_key(self):
        return ("ema", id(self), self.buffers, len(self._float_bufs))

    def state_tensors(self):
        return [self.ema_param] + [tb for tb, _sb in self._float_bufs] + [self.start_dev]

    def sync_hyper(self):
        """(decay, warmup) to the device when one changed (never inside a stream capture; ``FlatAdam.sync_hyper`` calls this)."""
        cur = (float(self.decay), float(self.warmup))
        if cur != self._hyper_host:
            self.hyper_dev.copy_(torch.tensor(cur, dtype=torch.float32))
            self._hyper_host = cur

    def _stats(self):
        return self.opt.stats_dev if self.opt.needs_norm() else None

    def launch(self, lo, hi):
        """The average on [lo, hi) of the flat buffers, on the current stream: right behind the step launch on that range."""
        opt = self.opt
        whole = (lo, hi) == (0, opt.numel)
        ops.flat_ema(self.ema_param if whole else self.ema_param[lo:hi], opt.flat_param if whole else opt.flat_param[lo:hi],
                     self.hyper_dev, opt.step_dev, self.start_dev, self._stats())

    def launch_buffers(self):
        """The float buffers in one launch (once per step, behind the last step launch)."""
        if self._table is not None:
            ops.ema_table(self._table, len(self._float_bufs), self.hyper_dev, self.opt.step_dev, self.start_dev, self._stats(),
                          self.buffers)
        ops.bump_stats_epoch()          # whatever rewrites running statistics must

    # ---------------------------------------------------------------------------------- the user's side
    def set_decay(self, decay):
        """A decay schedule: two floats in device memory change, no launch does - a recorded plan stays."""
        self.decay = check_decay(decay, "FlatEMA.set_decay")
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()

    def updates(self):
        """Updates applied since the attach / the last reset, as a device scalar (int32), no synchronisation."""
        return (self.opt.step_dev - self.start_dev)[0]

    def reset(self):
        """Teacher <- student again (parameters and buffers), and the warm-up starts over."""
        with torch.no_grad():
            self.ema_param.copy_(self.opt.flat_param)
            for tp, sp in self._frozen:
                tp.data.copy_(sp.data)
            for tb, sb in self._float_bufs:
                tb.copy_(sb)
            self.start_dev.copy_(self.opt.step_dev)
        self.sync_counters()
        ops.bump_param_epoch()
        ops.bump_stats_epoch()

    def sync_counters(self):
        """Integer buffers (``num_batches_tracked``) of the teacher <- the student's."""
        sd = self.model.state_dict()            # (folds the BatchNorm modules' pending step counts)
        with torch.no_grad():
            for k, tb in self._int_bufs:
                if k in sd:
                    tb.copy_(sd[k])

    def state_dict(self):
        self.sync_counters()
        return {"teacher": self.teacher.state_dict(), "decay": self.decay, "warmup": self.warmup, "buffers": self.buffers,
                "updates": int(self.updates().item())}

    def load_state_dict(self, state):
        decay = check_decay(state["decay"], "FlatEMA.load_state_dict")
        if state.get("buffers", self.buffers) != self.buffers:
            # (the mode selects a launch: part of launch_key(); a teacher saved with copied statistics is not one with averaged ones)
            raise ValueError(f"FlatEMA.load_state_dict: the state was saved with buffers={state['buffers']!r}, this average has "
                             f"buffers={self.buffers!r}; construct the FlatEMA with the saved mode")
        self.teacher.load_state_dict(state["teacher"])      # (copies into the views: ema_param keeps its place)
        self.decay, self.warmup = decay, bool(state["warmup"])
        with torch.no_grad():
            self.start_dev.copy_(self.opt.step_dev - int(state["updates"]))
        self.sync_hyper()
        ops.bump_param_epoch()
        ops.bump_stats_epoch()
