"""Host-side glue between PyTorch tensors (device memory, streams, autograd bookkeeping) and the HIP
kernels of libwsdl_hip.so.  Every arithmetic step runs in the library; torch here only allocates
buffers and orders calls on the current stream.  No CPU fallback: non-device tensors raise.
"""
import collections
import ctypes as C

import os

import threading

import numpy as np
import torch

from ._lib import lib, check, WsdlError

_vp = C.c_void_p


# torch.cuda.current_stream() builds a Stream object (and resolves the device twice) per call: ~6.5 us, ~350 times per
# training step = 2.3 ms of the host's ~13 ms (tools/host_profile.py).  The raw handle is one C call.
_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_device = torch._C._cuda_getDevice


def raw_stream(device=None):
    """hipStream_t of the current stream of ``device`` (default: the current device) as an int."""
    idx = device.index if (device is not None and device.index is not None) else _cur_device()
    return _raw_stream(idx)


def _stream():
    return _raw_stream(_cur_device())          # an int: the bound functions declare c_void_p (argtypes), ctypes converts


# ---- launch plans (plan.py; include/wsdl_hip.h "launch plans") ---------------------------------------------------------
# While a plan is being recorded, PLAN_REC[0] is the recording.  Everything the recorded launches touch must outlive the
# plan AT ITS ADDRESS: every tensor whose pointer is handed to the library meanwhile is kept by the recording (``_p``), so
# the caching allocator can never give its block to anybody else - no private memory pool needed.
# Both are PER HOST THREAD (as the C side's recording is: csrc/plan.hip): a second thread that uses the library while this
# one records - a loader worker, a second model - launches normally, pins nothing into this thread's recording and may
# record a plan of its own.
class _ThreadSlot(threading.local):
    """``slot[0]`` with one value per host thread."""

    def __init__(self, default):            # (threading.local calls this once per thread that touches the slot)
        self.v = default

    def __getitem__(self, i):
        return self.v

    def __setitem__(self, i, value):
        self.v = value


PLAN_REC = _ThreadSlot(None)


PLAN_REPLAYING = _ThreadSlot(False)     # a plan with host sections is being replayed (the sections run live, in their places)


def host_section(fn, *args):
    """Run ``fn(*args)`` - host work that must happen at THIS place of the launch sequence on every iteration and that a
    plan cannot hold: a collective of torch.distributed, a wait on its work handle, control-plane exchanges.  Outside a
    recording it is a plain call.  While a plan is being recorded the plan is cut here (``wsdl_plan_mark``), the
    recording pauses for the call, and a replay calls ``fn(*args)`` again between the two segments."""
    rec = PLAN_REC[0]
    if rec is None:
        return fn(*args)
    check(lib().wsdl_plan_mark(len(rec.sections)))
    check(lib().wsdl_plan_pause())
    PLAN_REC[0] = None
    try:
        return fn(*args)
    finally:
        PLAN_REC[0] = rec
        check(lib().wsdl_plan_resume())
        rec.sections.append((fn, args))


def _p(t):
    if t is None:
        return None
    rec = PLAN_REC[0]
    if rec is not None:
        rec.keep.append(t)
    return t.data_ptr()                                 # int -> c_void_p by the declared argtypes (no object per argument)


def _h(stream):
    """Raw hipStream_t (an int) of a torch stream object / of a raw handle."""
    return stream if isinstance(stream, int) else stream.cuda_stream


def stream_wait(waiter, waited):
    """``waiter`` waits for everything enqueued on ``waited`` so far (torch stream objects or raw handles).  Through the
    library (one event record + one stream wait), so that a plan being recorded sees the dependency."""
    check(lib().wsdl_stream_wait_stream(_h(waiter), _h(waited)))


class Event:
    """An event of the library (no timing).  ``record`` / ``wait`` default to torch's current stream; both are part of a plan
    being recorded (which then keeps the event alive)."""
    __slots__ = ("h", "__weakref__")

    def __init__(self):
        h = C.c_void_p()
        check(lib().wsdl_event_create(C.byref(h)))
        self.h = h.value

    def record(self, stream=None):
        if PLAN_REC[0] is not None:
            PLAN_REC[0].keep.append(self)
        check(lib().wsdl_event_record(self.h, _stream() if stream is None else _h(stream)))

    def wait(self, stream=None):
        if PLAN_REC[0] is not None:
            PLAN_REC[0].keep.append(self)
        check(lib().wsdl_stream_wait_event(_stream() if stream is None else _h(stream), self.h))

    def __del__(self):
        h, self.h = self.h, None
        if h:
            try:
                lib().wsdl_event_destroy(h)
            except Exception:       # interpreter shutdown
                pass


def cross_stream_use(t, stream):
    """``t`` lives on another stream's allocator pool and is used by work enqueued on ``stream`` (a torch stream object):
    keep the caching allocator from recycling it before that work has run."""
    t.record_stream(stream)
    if PLAN_REC[0] is not None:
        PLAN_REC[0].keep.append(t)


def memset_zero(t):
    """t.zero_() as a stream-ordered memset of the library (seen by a plan; ``t`` dense)."""
    if not t.is_contiguous():
        raise WsdlError("memset_zero: tensor is not dense")
    if torch.cuda.is_current_stream_capturing():
        return t.zero_()        # inside a hipGraph capture: the tensor library's fill kernel, as the captured graphs always had
    check(lib().wsdl_memset_async(_p(t), 0, t.numel() * t.element_size(), _stream()))
    return t


def add_int(t, delta=1):
    """t += delta for a one-element device int32 / int64 (Adam's step number, a dropout call counter) - a launch of the
    library instead of torch's ``add_`` (a plan records launches of this library only)."""
    if t.numel() != 1 or t.dtype not in (torch.int32, torch.int64):
        raise WsdlError("add_int: a one-element int32 / int64 device tensor")
    check(lib().wsdl_add_int(_p(t), int(t.dtype == torch.int64), int(delta), _stream()))
    return t


def clamp_max_labels(labels, hi=1):
    """torch.clamp(labels, max=hi) for int64 device labels (reference SegmentationModel.py:100); other dtypes / host
    tensors take torch's own clamp."""
    if not labels.is_cuda or labels.dtype != torch.int64:
        return torch.clamp(labels, max=hi)
    labels = labels.contiguous()
    out = torch.empty_like(labels)
    if labels.numel():
        check(lib().wsdl_clamp_max_i64(_p(labels), _p(out), labels.numel(), int(hi), _stream()))
    return out


def _req(t, name="tensor", dtype=torch.float32):
    if not t.is_cuda:
        raise WsdlError(f"{name}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
    if t.dtype != dtype:
        raise WsdlError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def _dense(t, name="tensor"):
    _req(t, name)
    return t if t.is_contiguous() else t.contiguous()


def _planes(t, name="tensor"):
    """(tensor, batch_stride): accept NCHW tensors whose images are dense but batch stride is larger
    (channel slices of a concatenated tensor) without copying; anything else is made contiguous."""
    _req(t, name)
    B, Cc, H, W = t.shape
    if t.is_contiguous():
        return t, Cc * H * W
    st = t.stride()
    if st[3] == 1 and st[2] == W and st[1] == H * W and st[0] >= Cc * H * W:
        return t, st[0]
    t = t.contiguous()
    return t, Cc * H * W


_ws_cache = {}

# Parameters / BN statistics are also written by raw-pointer kernels (Adam step, train-mode running statistics),
# which torch's tensor version counters cannot see.  Every such writer bumps PARAM_EPOCH; eval-mode caches of
# derived tensors (re-laid-out weights, folded BN scale/shift) are keyed on (PARAM_EPOCH, tensor._version, data_ptr).
PARAM_EPOCH = [0]      # parameters rewritten by the Adam kernel
STATS_EPOCH = [0]      # BN running statistics rewritten by a train-mode forward


def bump_param_epoch():
    PARAM_EPOCH[0] += 1


def bump_stats_epoch():
    STATS_EPOCH[0] += 1


def _cache_key(*tensors):
    return (PARAM_EPOCH[0], STATS_EPOCH[0]) + tuple((t._version, t.data_ptr()) for t in tensors)


def _weight_key(w):
    return (PARAM_EPOCH[0], w._version, w.data_ptr())


def _cached_prep(cache, weight, need_dx):
    """(wt_fwd, wt_dgrad) from the module cache when the weights have not changed since they were laid out (eval
    mode, or prefetched on the side stream right after the optimiser step); otherwise lay them out now."""
    if cache is not None and cache.get("prep_key") == _weight_key(weight) and (cache["prep"][1] is not None or not need_dx):
        ev = cache.get("prep_event")
        if ev is not None:
            ev.wait()
        if PLAN_REC[0] is not None:
            PLAN_REC[0].keep.append(cache["prep"])
        return cache["prep"]
    wf, wd = prep_weights(weight, True, need_dx)
    if cache is not None:
        cache["prep_key"], cache["prep"], cache["prep_event"] = _weight_key(weight), (wf, wd), None
    return wf, wd


_PREFETCH_HEAD = int(os.environ.get("WSDL_PREFETCH_HEAD", "12"))    # convolutions of the first re-layout batch after an optimiser step (stem + layer1)
LAYOUT_EPOCH = [0]     # bumped by options that change what a layout buffer holds / how large it is


_prep_streams = {}


def _norm_device(device):
    """torch.device with an explicit index: the stream tables and the census must agree on the key (an index-less
    ``torch.device('cuda')`` used to create streams the census did not count)."""
    device = device if isinstance(device, torch.device) else torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", _cur_device())
    return device


def prep_stream(device):
    """Third stream: re-layouts that follow an early segment step must not sit in the side stream in front of the weight
    gradients (and the Adam launches) still to come."""
    if device.index is None:
        device = _norm_device(device)
    st = _prep_streams.get(device)
    if st is None:
        st = _prep_streams[device] = torch.cuda.Stream(device=device)
    return st


def prefetch_weight_layouts(convs, use_events=True, epoch_ahead=0, pingpong=False, after=None, _head=True):
    """Lay out next step's weights on the side stream (called right after the optimiser step of these weights): the
    re-layout kernels leave the forward chain; each conv waits on its own event (``use_events=False``: the main stream
    joins the side stream instead - inside a captured graph).
    ``epoch_ahead``: the caller will bump the parameter epoch this many times before the layouts are used (early
    segment steps run before ``FlatAdam.step`` does).  ``after``: an event (the segment's Adam launch) - the re-layouts then
    run on the prep stream behind it instead of on the side stream.  ``pingpong``: write into the conv's spare pair of buffers and swap -
    input-gradient kernels of the CURRENT step that are still to be enqueued keep reading the pair they were given."""
    if not convs:
        return
    dev = convs[0].weight.device
    main, side = _stream(), side_stream(dev)
    if _head and _PREFETCH_HEAD > 0 and len(convs) > 2 * _PREFETCH_HEAD:
        # the forward that follows waits for its FIRST layers' layouts: give those their own (small) amax launch instead of
        # queueing them behind the amax pass over all 158 MB of weights (105 us before the next step could start)
        prefetch_weight_layouts(convs[:_PREFETCH_HEAD], use_events, epoch_ahead, pingpong, after, False)
        return prefetch_weight_layouts(convs[_PREFETCH_HEAD:], use_events, epoch_ahead, pingpong, after, False)
    if after is not None and use_events:
        side = prep_stream(dev)
        after.wait(side)
    else:
        stream_wait(side, main)
    ev = None
    cache0 = convs[0].__dict__.setdefault("_wsdl_cache", {})
    with torch.cuda.stream(side):
        amaxes = multi_amax([m.weight for m in convs], persistent=True) if CONV_ARITH[0] == 1 else None
        batch = []          # convolutions whose existing split layouts are rewritten by ONE launch (after the loop)
        for i, m in enumerate(convs):
            cache = m.__dict__.setdefault("_wsdl_cache", {})
            fresh = cache.get("prep_layout") == LAYOUT_EPOCH[0]
            old = cache.get("prep") if fresh else None
            target = (cache.get("prep_spare") if fresh else None) if pingpong else old
            w = m.weight
            in_batch = (MULTI_PREP[0] and amaxes is not None and target is not None and target[0] is not None
                        and target[1] is not None and w.is_contiguous() and _both_split(w))
            ev = None
            if in_batch:
                wf, wd = target
                batch.append((w, wf, wd, amaxes[i:i + 1], cache))
            else:
                wf, wd = prep_weights(w, True, True, amaxes[i:i + 1] if amaxes is not None else None, reuse=target)
                if use_events:
                    ev = cache.get("own_event")         # one event per site, re-recorded step after step
                    if ev is None:
                        ev = cache["own_event"] = Event()
                    ev.record(side)
            cache["prep_key"] = (PARAM_EPOCH[0] + epoch_ahead, w._version, w.data_ptr())
            cache["prep"], cache["prep_event"] = (wf, wd), ev
            cache["prep_spare"] = old if pingpong else None
            cache["prep_layout"] = LAYOUT_EPOCH[0]
        if batch and torch.cuda.is_current_stream_capturing() and not prep_weights_multi([b[:4] for b in batch], lookup_only=True):
            # a capture cannot copy a new descriptor table to the device: launch them one by one (as before)
            for w, wf, wd, a, _c in batch:
                prep_weights(w, True, True, a, reuse=(wf, wd))
            batch = []
        if batch:
            prep_weights_multi([b[:4] for b in batch])
            if use_events:
                ev = cache0.get("batch_event")
                if ev is None:
                    ev = cache0["batch_event"] = Event()
                ev.record(side)
                for b in batch:
                    b[4]["prep_event"] = ev
            else:
                ev = None
    if not use_events:
        stream_wait(main, side)         # graph capture: no cross-replay events - the step ends with the layouts complete
    return ev                           # recorded behind the last re-layout (None without events)


def _stream_object(device, handle):
    """The torch stream object behind a raw handle of one of the library's streams (None: not one of them)."""
    for st in library_streams(device):
        if st.cuda_stream == handle:
            return st
    return None


def workspace(nbytes, device, stream=None):
    """Stream-ordered scratch: one growing buffer per (device, stream).  ``stream``: a raw handle (default: the current one).
    A buffer is allocated with ITS stream current, so that the caching allocator files it under that stream's pool: when a
    larger geometry replaces it, the old block can only be handed to later allocations of the same stream - behind the
    kernels still queued there that write it (a side-stream workspace allocated from the main stream's pool could be given
    to the next main-stream tensor while side-stream weight gradients were still filling it)."""
    cur = raw_stream(device)
    key = (device, cur if stream is None else stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        n = max(int(nbytes), 1 << 20)
        if stream is None or stream == cur:
            buf = torch.empty(n, dtype=torch.uint8, device=device)
        else:
            obj = _stream_object(device, stream)
            if obj is None:
                raise WsdlError("workspace: a stream handle that is not one of the library's streams")
            with torch.cuda.stream(obj):
                buf = torch.empty(n, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


_size_cache = {}      # (query, geometry) -> bytes: pure functions of the geometry under a fixed option set (cleared by set_option)


def _ws_bytes(query, *geom):
    key = (query, geom)
    n = _size_cache.get(key)
    if n is None:
        n = _size_cache[key] = getattr(lib(), query)(*geom)
    return n


def conv_out_hw(H, W, k, stride, pad, dil):
    return ((H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1)


# ------------------------------------------------------------------------------------------ raw ops
CONV_ARITH = [1]       # mirrors the library's "conv_arith": 1 = fp16x2 split kernels (need per-tensor amax scalars)


def set_option(name, value):
    """wsdl_set_option + invalidation of every cached weight layout (options such as "conv_split" change what the
    layout buffers hold)."""
    check(lib().wsdl_set_option(name.encode(), int(value)))
    if name == "conv_arith":
        CONV_ARITH[0] = int(value != 0)
    _both_split_cache.clear()          # what the library answered under the old option set
    _size_cache.clear()
    LAYOUT_EPOCH[0] += 1
    bump_param_epoch()


def launch_trace(on):
    """wsdl_launch_trace: the convolution entry points describe every launch they choose (form, tile, K slices, XCD order,
    bands, grid) - read back with ``last_launches()``."""
    check(lib().wsdl_launch_trace(int(bool(on))))


def last_launches():
    """This thread's launch descriptions since the previous call (a "; "-separated string)."""
    return lib().wsdl_last_launches().decode()


# ---- per-tensor amax scalars ------------------------------------------------------------------------------------
# The fp16x2 convolution kernels scale each operand tensor by a power of two derived from a device scalar
# amax >= max|tensor| (conv_split.h).  The kernel that WRITES a tensor publishes it for free (BatchNorm forward /
# backward, the eval-mode conv epilogue: an atomicMax into a zeroed slot); the tensor carries it as ``_wsdl_amax``.
# Tensors that arrive without one (the network input, concatenations, dropout outputs, views) get a read pass
# (``wsdl_amax``) the first time a split convolution consumes them.
_amax_pools = {}
AMAX_POOL_SLOTS = [4096]      # slots per pool (tests shrink it to force roll-overs)


def amax_slot(device):
    """A zero-initialised one-element fp32 view (slots are handed out once; a pool of 4096 is one memset).

    One pool per (device, STREAM), like ``workspace()``: the pool's memset is ordered on the stream that allocates it,
    and a slot's first use - the producing kernel's atomicMax into the zeroed slot - is enqueued on that same stream,
    so a roll-over on one stream (a CAM lane, the side stream's aux head) can neither wipe nor pre-date a slot another
    stream is publishing into.  Consumers on other streams read a slot only behind the stream join that orders them
    after its producer (the weight-gradient kernels on the side stream: ``side.wait_stream(main)``)."""
    key = (device, raw_stream(device))
    pool = _amax_pools.get(key)
    if pool is None or pool[1] >= AMAX_POOL_SLOTS[0]:
        # a slot is a PAIR of floats: [max|tensor|, ~bits of the smallest non-zero channel maximum] - the second one is written
        # by the BatchNorm kernels only (range sentinel, include/wsdl_hip.h wsdl_range_check); callers see the first
        buf = memset_zero(torch.empty(2 * AMAX_POOL_SLOTS[0], device=device, dtype=torch.float32))
        if not torch.cuda.is_current_stream_capturing():
            # slots are read by kernels on the other streams of this library (weight gradients on the side stream, the
            # main stream joining a CAM lane): keep the caching allocator from recycling a retired pool under them
            for st in library_streams(device):
                buf.record_stream(st)
            buf.record_stream(torch.cuda.default_stream(device))
        pool = [buf, 0]
        _amax_pools[key] = pool
    i = pool[1]
    pool[1] += 1
    return pool[0][2 * i:2 * i + 1]


RANGE_LIMIT_LOG2 = 25          # a tensor whose channel maxima spread further than 2^25 leaves the fp16x2 arithmetic's safe range
_range_out = {}
_range_rows = {}               # device -> rows of _range_out the latest range_check writes
_RANGE_ROWS = 8
_range_warned_pools = [False]


def range_check(device):
    """Reduce the (max, min channel maximum) pairs of the amax slots handed out on ``device`` since their pools were created
    (launches of the library on the current stream; no host synchronisation): ``range_status`` reads the result later."""
    device = _norm_device(device)
    pools = [(k, v) for k, v in _amax_pools.items() if k[0] == device and v[1] > 0]
    if not pools:
        return
    out = _range_out.get(device)
    if out is None:
        out = _range_out[device] = torch.zeros(_RANGE_ROWS, 3, dtype=torch.float32).pin_memory()
    if len(pools) > _RANGE_ROWS and not _range_warned_pools[0]:
        _range_warned_pools[0] = True
        import warnings
        warnings.warn(f"range_check: {len(pools)} amax pools on {device}, only the first {_RANGE_ROWS} are checked "
                      "(one pool per stream that requested slots: more streams than the library creates)")
    pools = pools[:_RANGE_ROWS]
    # the check kernels run on the CURRENT stream: a pool that belongs to another stream (the side stream's aux head, a LayerCAM
    # lane) is only read once that stream has been joined - FlatAdam.step() calls this behind join_side_stream; a pool of a
    # stream the caller did not join may still be written while it is read, so it is left out
    cur = raw_stream(device)
    joined = {cur, _side_streams[device].cuda_stream if device in _side_streams else cur}
    pools = [(k, v) for k, v in pools if k[1] in joined]
    for j, (_k, (buf, used)) in enumerate(pools):
        check(lib().wsdl_range_check(_p(buf), int(used), RANGE_LIMIT_LOG2, _p(out[j]), _stream()))
    _range_rows[device] = len(pools)      # rows beyond hold an earlier call's figures: range_status does not read them


def range_status(device):
    """What the last completed ``range_check`` found: {"worst_log2", "pairs_over_limit", "pairs_seen", "exceeded"} - read from
    host memory the check kernels write; a step old at most."""
    out = _range_out.get(_norm_device(device))
    if out is None:
        return {"worst_log2": 0.0, "pairs_over_limit": 0, "pairs_seen": 0, "exceeded": False, "limit_log2": RANGE_LIMIT_LOG2}
    a = out.numpy()[:_range_rows.get(_norm_device(device), 0)]      # a view of the pinned buffer (polled after every replayed step: a few microseconds)
    if a.shape[0] == 0:
        return {"worst_log2": 0.0, "pairs_over_limit": 0, "pairs_seen": 0, "exceeded": False, "limit_log2": RANGE_LIMIT_LOG2}
    over = int(a[:, 1].sum())
    return {"worst_log2": float(a[:, 0].max()), "pairs_over_limit": over, "pairs_seen": int(a[:, 2].sum()), "exceeded": over > 0,
            "limit_log2": RANGE_LIMIT_LOG2}


_lane_streams = {}     # device -> the library's streams beyond the side and the prep stream (LayerCAM lanes 2, 3, ...)


def lane_stream(device, i):
    """The i-th extra stream of the library on ``device``.  A ROCm process has four hardware queues by default and HIP
    streams beyond them share one (their work then runs one behind the other): a training step that has run in the process
    holds the side stream (and possibly the prep stream), so LayerCAM lanes with streams of their own made three batches in
    flight take 0.27 ms/img instead of 0.185.  Lanes 0 and 1 therefore ARE the side and the prep stream; only further
    lanes create streams, once per device whatever the number of generators."""
    device = _norm_device(device)
    if i == 0:
        return side_stream(device)
    if i == 1:
        return prep_stream(device)
    more = _lane_streams.setdefault(device, [])
    while len(more) < i - 1:
        if stream_census(device)["total"] >= MAX_HW_QUEUES:
            # no fifth stream: it would share a hardware queue with one of the four (and, in a data-parallel process, slow the
            # gradient collectives or the weight gradients down with it).  Further lanes take turns on the side / prep stream.
            return (side_stream(device), prep_stream(device))[i % 2]
        more.append(torch.cuda.Stream(device=device))
    return more[i - 2]


MAX_HW_QUEUES = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))     # hardware queues of a ROCm process (the runtime's own switch)


def stream_census(device):
    """The streams this process keeps busy on ``device``: torch's current (default) stream, the library's side / prep / lane
    streams, and - once a process group with the nccl (RCCL) backend exists - the stream RCCL enqueues its collectives on.
    A ROCm process has ``MAX_HW_QUEUES`` hardware queues (4); a stream beyond them shares one, i.e. runs behind another
    stream's work (measured: three LayerCAM lanes 0.185 -> 0.27 ms/img with a fifth stream in use, profiles/r03_notes.md).
    ``lane_stream`` refuses to create the fifth; tests/test_hip_dp.py checks the count in a data-parallel process."""
    device = _norm_device(device)
    c = {"main": 1, "side": int(device in _side_streams), "prep": int(device in _prep_streams),
         "lanes": len(_lane_streams.get(device, [])), "rccl": 0}
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            c["rccl"] = 1
    except Exception:        # a process group that is being torn down
        pass
    c["total"] = sum(c.values())
    c["hw_queues"] = MAX_HW_QUEUES
    return c


def library_streams(device):
    """Every stream this library has created on ``device`` (amax slots may be read on any of them)."""
    device = _norm_device(device)
    return [st for st in (_side_streams.get(device), _prep_streams.get(device)) if st is not None] + list(_lane_streams.get(device, []))


def _publish_amax(t, slot):
    """Attach a producer-published amax scalar to the tensor it bounds, with the tensor's version: a later in-place
    modification (``t.mul_()``, ``buf.copy_()``) makes ``amax_of`` measure again instead of trusting a stale bound."""
    t._wsdl_amax = slot
    t._wsdl_amax_version = t._version


def _publish_camax(t, camax, presplit=None):
    """Attach producer-published per-channel maxima (and, for a BatchNorm input gradient, its pre-split fp16 rows) to the
    tensor they describe, with the tensor's version - as ``_publish_amax``: after an in-place modification ``camax_of``
    answers None and the weight gradient falls back to the per-tensor scale ``amax_of`` measures again."""
    t._wsdl_camax = camax
    if presplit is not None:
        t._wsdl_presplit = presplit
    t._wsdl_camax_version = t._version


def camax_of(t, presplit=False):
    """The per-channel maxima the tensor's producer published, or None if it carries none or was modified in place since
    (``y.mul_()``, ``copy_()``: a channel that grew would overflow the fp16 pieces, pre-split rows would hold the old values).
    ``presplit=True``: the pair (maxima, pre-split rows or None) - the rows are only valid together with the maxima."""
    c = getattr(t, "_wsdl_camax", None)
    if c is not None and getattr(t, "_wsdl_camax_version", None) != t._version:
        c = None
    if not presplit:
        return c
    return c, (getattr(t, "_wsdl_presplit", None) if c is not None else None)


def reset_amax_pool(device):
    """Forget the current slot pools of ``device``: the next request allocates (and zeroes) a new one - graph.py brackets a
    capture with it so that the captured step's slots are re-zeroed by every replay."""
    device = device if isinstance(device, torch.device) else torch.device(device)
    for key in [k for k in _amax_pools if k[0] == device]:
        _amax_pools.pop(key, None)


def _split_kc(kc, taps):
    """Could a convolution contracting ``kc`` channels over ``taps`` taps run on the split kernels? (split_eligible in
    conv_igemm.hip; an over-approximation only costs an unused amax)."""
    return CONV_ARITH[0] == 1 and kc % 16 == 0 and taps <= 9


def amax_of(t, needed=True):
    """The tensor's amax scalar: the one its producer published, else one read pass (cached on the tensor)."""
    if not needed:
        return None
    a = getattr(t, "_wsdl_amax", None)
    if a is not None and getattr(t, "_wsdl_amax_version", t._version) != t._version:
        a = None                 # modified in place since the bound was taken (copy_ into a reused buffer, mul_): measure again
    if a is None:
        tt, bs = _planes(t, "amax input") if t.dim() == 4 else (_dense(t, "amax input"), 0)
        a = amax_slot(t.device)
        B = tt.shape[0] if tt.dim() == 4 else 1
        per = tt.numel() // B
        check(lib().wsdl_amax(_p(tt), B, per, bs if tt.dim() == 4 else per, _p(a), 0, _stream()))    # the slot is zeroed
        try:
            t._wsdl_amax = a
            t._wsdl_amax_version = t._version
        except AttributeError:
            pass
    return a


def _layout_buffer(w, dgrad):
    import ctypes
    Cout, Cin, kh, kw = w.shape
    plain = ctypes.c_int(0)
    nbytes = lib().wsdl_conv2d_weight_layout_bytes(Cout, Cin, kh, kw, int(dgrad), ctypes.byref(plain))
    if plain.value and dgrad and kh * kw == 1:
        return w.detach().reshape(Cout, Cin), False        # [tap*Cout+co][ci] of a 1x1 kernel IS w's own layout
    return torch.empty(nbytes // 4, device=w.device, dtype=torch.float32), True


def prep_weights(w, want_fwd=True, want_dgrad=True, w_amax=None, reuse=None):
    """Opaque layout buffers (wt_fwd, wt_dgrad) for conv2d_fwd / conv2d_dgrad (include/wsdl_hip.h).  ``w_amax``: device
    scalar max|w| if the caller already has it (``multi_amax``); otherwise the library reduces it.  ``reuse``: a
    previous (wt_fwd, wt_dgrad) pair of this weight to overwrite in place (the per-step re-layout keeps its buffers:
    no allocator churn, and a captured graph keeps reading the addresses it was captured with)."""
    w = _dense(w, "weight")
    Cout, Cin, kh, kw = w.shape
    if reuse is not None and reuse[0] is not None and (reuse[1] is not None or not want_dgrad):
        wf, wd = reuse
        make_wd = wd is not None and wd.data_ptr() != w.data_ptr()
        check(lib().wsdl_conv2d_prep_weights(_p(w), _p(wf), _p(wd if make_wd else None), Cout, Cin, kh, kw, _p(w_amax),
                                             _stream()))
        return wf, wd
    wf = _layout_buffer(w, False)[0] if want_fwd else None
    wd, make_wd = _layout_buffer(w, True) if want_dgrad else (None, False)
    if want_fwd or make_wd:
        check(lib().wsdl_conv2d_prep_weights(_p(w), _p(wf), _p(wd if make_wd else None), Cout, Cin, kh, kw, _p(w_amax),
                                             _stream()))
    return wf, wd


_multi_amax_cache = {}


def multi_amax(tensors, persistent=False):
    """max|t| of every tensor of a FIXED list in one launch -> (n,) device tensor.  The pointer / count tables live on
    the device and are built once per list (parameters keep their addresses inside the flat optimiser buffer).
    ``persistent``: the result goes into one buffer per list, overwritten by the next call (stream-ordered consumers only)."""
    key = tuple((t.data_ptr(), t.numel()) for t in tensors)
    ent = _multi_amax_cache.get(key)
    dev = tensors[0].device
    if ent is None:
        ptrs = torch.tensor([k[0] for k in key], dtype=torch.int64).to(dev)
        counts = torch.tensor([k[1] for k in key], dtype=torch.int64).to(dev)
        ent = _multi_amax_cache[key] = (ptrs, counts, torch.empty(len(tensors), device=dev, dtype=torch.float32))
        if len(_multi_amax_cache) > 64:
            _multi_amax_cache.pop(next(iter(_multi_amax_cache)))
    out = ent[2] if persistent else torch.empty(len(tensors), device=dev, dtype=torch.float32)
    check(lib().wsdl_multi_amax(_p(ent[0]), _p(ent[1]), len(tensors), _p(out), _stream()))
    return out


MULTI_PREP = [os.environ.get("WSDL_MULTI_PREP", "1") != "0"]      # the per-step re-layout of all split layouts in one launch
_both_split_cache = {}
_prep_tables = {}


def _both_split(w):
    """Are the forward and the dgrad layout of this weight both split layouts (what wsdl_conv2d_prep_weights_multi takes)?"""
    import ctypes
    key = tuple(w.shape)
    r = _both_split_cache.get(key)
    if r is None:
        Cout, Cin, kh, kw = key
        pf, pd = ctypes.c_int(0), ctypes.c_int(0)
        lib().wsdl_conv2d_weight_layout_bytes(Cout, Cin, kh, kw, 0, ctypes.byref(pf))
        lib().wsdl_conv2d_weight_layout_bytes(Cout, Cin, kh, kw, 1, ctypes.byref(pd))
        r = _both_split_cache[key] = (pf.value == 0 and pd.value == 0 and kh * kw <= 9)
    return r


class _PrepDesc(C.Structure):
    _fields_ = [("w", C.c_void_p), ("wt_fwd", C.c_void_p), ("wt_dgrad", C.c_void_p), ("w_amax", C.c_void_p),
                ("Cout", C.c_int), ("Cin", C.c_int), ("taps", C.c_int), ("grid_x", C.c_int),
                ("block_begin", C.c_int), ("reserved", C.c_int)]


def prep_weights_multi(entries, lookup_only=False):
    """entries: [(weight, wt_fwd, wt_dgrad, w_amax (1,) device tensor)] with existing layout buffers, all ``_both_split``:
    one launch re-lays them all out (include/wsdl_hip.h wsdl_conv2d_prep_weights_multi).  The descriptor table goes to the
    device once per set of addresses (weights live in the flat optimiser buffer, layout buffers are reused step after step)."""
    key = tuple((w.data_ptr(), wf.data_ptr(), wd.data_ptr(), a.data_ptr()) for w, wf, wd, a in entries)
    ent = _prep_tables.get(key)
    if lookup_only:
        return ent is not None
    if ent is None:
        arr = (_PrepDesc * len(entries))()
        blocks = 0
        for d, (w, wf, wd, a) in zip(arr, entries):
            Cout, Cin, kh, kw = w.shape
            d.w, d.wt_fwd, d.wt_dgrad, d.w_amax = w.data_ptr(), wf.data_ptr(), wd.data_ptr(), a.data_ptr()
            d.Cout, d.Cin, d.taps, d.grid_x, d.block_begin = Cout, Cin, kh * kw, (Cin + 31) // 32, blocks
            blocks += d.grid_x * ((Cout + 31) // 32)
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(entries[0][0].device)
        ent = _prep_tables[key] = (table, len(entries), blocks)
        if len(_prep_tables) > 64:
            _prep_tables.pop(next(iter(_prep_tables)))
    check(lib().wsdl_conv2d_prep_weights_multi(_p(ent[0]), ent[1], ent[2], _stream()))


def conv2d_fwd(x, wt_fwd, wshape, stride, pad, dil, scale=None, shift=None, residual=None, relu=False, out=None,
               x_amax=None, want_amax=False, y_amax=None):
    """``x_amax``: the input's amax scalar (looked up / computed when None and the split kernels may run);
    ``want_amax``: publish max|out| as ``out._wsdl_amax`` (the output feeds another convolution directly);
    ``y_amax``: an existing slot to publish into instead of a fresh one (producers of the slices of one buffer share it)."""
    if x_amax is None:
        x_amax = amax_of(x, _split_kc(x.shape[1], wshape[2] * wshape[3]))
    x, x_bs = _planes(x, "x")
    B, Cin, H, W = x.shape
    Cout, Cin2, kh, kw = wshape
    if Cin2 != Cin:
        raise WsdlError(f"conv2d: input has {Cin} channels, weight expects {Cin2}")
    OH, OW = conv_out_hw(H, W, kh, stride, pad, dil)
    if OH <= 0 or OW <= 0:
        raise WsdlError(f"conv2d: empty output ({OH} x {OW})")
    if out is None:
        out = torch.empty(B, Cout, OH, OW, device=x.device, dtype=torch.float32)
        y_bs = Cout * OH * OW
    else:
        out, y_bs = _planes(out, "out")
        if tuple(out.shape) != (B, Cout, OH, OW):
            raise WsdlError("conv2d: bad preallocated output shape")
    res_bs = 0
    if residual is not None:
        residual, res_bs = _planes(residual, "residual")
        if tuple(residual.shape) != (B, Cout, OH, OW):
            raise WsdlError("conv2d: residual shape mismatch")
    nws = _ws_bytes("wsdl_conv2d_igemm_workspace", B, Cin, H, W, Cout, kh, kw, stride, pad, dil, 0)
    ws = workspace(nws, x.device) if nws else None
    if y_amax is None:
        y_amax = amax_slot(x.device) if (want_amax and CONV_ARITH[0] == 1) else None
    check(lib().wsdl_conv2d_fwd(_p(x), _p(wt_fwd), _p(out), B, Cin, H, W, Cout, kh, kw, stride, pad, dil,
                                _p(scale), _p(shift), _p(residual), int(relu), x_bs, y_bs, res_bs, _p(x_amax), _p(y_amax),
                                _p(ws), ws.numel() if ws is not None else 0, _stream()))
    if y_amax is not None:
        _publish_amax(out, y_amax)
    return out


def conv2d_dgrad(dy, wt_dgrad, wshape, xshape, stride, pad, dil, accumulate_into=None, dy_amax=None, acc_mask=None):
    """``accumulate_into``: dx = dgrad + that tensor, in place.  ``acc_mask`` (bits from ``bn_train_fwd(want_mask=True)``, same
    shape as dx): only the elements of ``accumulate_into`` whose bit is set count (the masked gradient of an identity branch)."""
    if acc_mask is not None and (accumulate_into is None or acc_mask.dtype != torch.uint8
                                 or acc_mask.numel() * 8 != accumulate_into.numel() or not accumulate_into.is_contiguous()):
        raise WsdlError("conv2d_dgrad: acc_mask needs a dense accumulate_into tensor of 8 x its number of bytes")
    if dy_amax is None:
        dy_amax = amax_of(dy, _split_kc(wshape[0], wshape[2] * wshape[3]))
    dy, dy_bs = _planes(dy, "dy")
    B, Cin, H, W = xshape
    Cout, _, kh, kw = wshape
    dx = accumulate_into if accumulate_into is not None else torch.empty(xshape, device=dy.device, dtype=torch.float32)
    nws = _ws_bytes("wsdl_conv2d_igemm_workspace", B, Cin, H, W, Cout, kh, kw, stride, pad, dil, 1)
    ws = workspace(nws, dy.device) if nws else None
    check(lib().wsdl_conv2d_dgrad(_p(dy), _p(wt_dgrad), _p(dx), B, Cin, H, W, Cout, kh, kw, stride, pad, dil,
                                  int(accumulate_into is not None), _p(acc_mask), dy_bs, _p(dy_amax), _p(ws),
                                  ws.numel() if ws is not None else 0, _stream()))
    dx._wsdl_fresh = True        # a buffer this library has just produced and nobody else holds (see _owned)
    return dx


def fwd_group_ok(n, xshape, cout):
    """Does the library serve ``n`` forward convolutions of one input of ``xshape`` as one grouped launch?"""
    B, Cin, H, W = xshape
    return bool(lib().wsdl_conv2d_fwd_group_ok(int(n), B, Cin, H, W, int(cout)))


def conv2d_fwd_group(x, wfs, wshapes, dils, x_amax=None, outs=None):
    """[conv(x, w_i)] for 1x1 / 3x3 stride-1 'same' convolutions of ONE input in one launch (include/wsdl_hip.h
    wsdl_conv2d_fwd_group): raw outputs, no epilogue."""
    n = len(wfs)
    if x_amax is None:
        x_amax = amax_of(x, _split_kc(x.shape[1], 9))
    x, x_bs = _planes(x, "x")
    B, Cin, H, W = x.shape
    Cout = wshapes[0][0]
    if any(ws[0] != Cout or ws[1] != Cin for ws in wshapes):
        raise WsdlError("conv2d_fwd_group: the problems must share their channel counts")
    IA, PA, LA = C.c_int * n, _vp * n, C.c_longlong * n
    ks, ds = IA(*[int(ws[2]) for ws in wshapes]), IA(*[int(d) for d in dils])
    nws = lib().wsdl_conv2d_fwd_group_workspace(n, ks, ds, B, Cin, H, W, Cout)
    if nws == 0:
        raise WsdlError("conv2d_fwd_group: geometry not supported")
    ws = workspace(nws, x.device)
    if outs is None:
        outs = [torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32) for _ in range(n)]
    bss = []
    dense = []
    for o in outs:
        t, bs = _planes(o, "out")
        if t is not o:
            raise WsdlError("conv2d_fwd_group: preallocated outputs must be dense planes")
        dense.append(t)
        bss.append(bs)
    check(lib().wsdl_conv2d_fwd_group(n, _p(x), PA(*[_p(w) for w in wfs]), PA(*[_p(t) for t in dense]), ks, ds, B, Cin, H, W,
                                      Cout, x_bs, LA(*bss), _p(x_amax), _p(ws), ws.numel(), _stream()))
    return outs


def dgrad_multi_ok(n, xshape, cout):
    """Does the library serve the one-launch input gradient of ``n`` convolutions over an input of ``xshape``?"""
    B, Cin, H, W = xshape
    return bool(lib().wsdl_conv2d_dgrad_multi_ok(int(n), B, Cin, H, W, int(cout)))


def conv2d_dgrad_multi(dys, wds, wshapes, dils, xshape, accumulate_into=None, dy_amaxes=None):
    """dx = [accumulate_into +] sum_i dgrad(dys[i], wds[i]) in ONE launch (include/wsdl_hip.h wsdl_conv2d_dgrad_multi):
    convolutions of the same input, 1x1 / 3x3, stride 1, 'same' padding.  The first source decides the column bands of
    the padding-tap skipping."""
    n = len(dys)
    B, Cin, H, W = xshape
    Cout = wshapes[0][0]
    amaxes = []
    dense = []
    bss = []
    for i in range(n):
        if wshapes[i][0] != Cout or wshapes[i][1] != Cin:
            raise WsdlError("conv2d_dgrad_multi: the sources must share their channel counts")
        a = dy_amaxes[i] if dy_amaxes is not None and dy_amaxes[i] is not None else \
            amax_of(dys[i], _split_kc(Cout, wshapes[i][2] * wshapes[i][3]))
        t, bs = _planes(dys[i], "dy")
        amaxes.append(a)
        dense.append(t)
        bss.append(bs)
    dx = accumulate_into if accumulate_into is not None else torch.empty(xshape, device=dys[0].device, dtype=torch.float32)
    PA, IA, LA = _vp * n, C.c_int * n, C.c_longlong * n
    check(lib().wsdl_conv2d_dgrad_multi(n, PA(*[_p(t) for t in dense]), PA(*[_p(w) for w in wds]), PA(*[_p(a) for a in amaxes]),
                                        IA(*[int(ws[2]) for ws in wshapes]), IA(*[int(d) for d in dils]), LA(*bss), _p(dx),
                                        B, Cin, H, W, Cout, int(accumulate_into is not None), _stream()))
    dx._wsdl_fresh = True
    return dx


def _wgrad_split(wshape):
    """May the library's fp16x2 weight-gradient kernel take this shape (then both operands need amax scalars - a read
    pass on the main stream for a tensor that carries none, so this must not claim more than the library's own rule)."""
    return CONV_ARITH[0] == 1 and wshape[0] % 128 == 0 and wshape[1] % 128 == 0


def wgrad_presplit_bytes(xshape, wshape, stride, pad, dil):
    """Bytes of the pre-split dY rows the weight gradient of this convolution reads when its producer writes them
    (``bn_train_bwd(presplit_bytes=)``); 0 where it would not use them."""
    B, Cin, H, W = xshape
    Cout, _, kh, kw = wshape
    return _ws_bytes("wsdl_conv2d_wgrad_presplit_bytes", B, Cin, H, W, Cout, kh, kw, stride, pad, dil)


def conv2d_wgrad(x, dy, wshape, stride, pad, dil, out=None, accumulate=False, x_amax=None, dy_amax=None, stream=None,
                 x_camax=None, dy_camax=None, dy_presplit=None):
    """``stream``: raw handle of the stream to launch on (default: the current stream) - the side-stream launches of the
    training step pass it instead of switching torch's current stream (a ``with torch.cuda.stream()`` costs the host ~20 us,
    61 times per step).  ``x_camax`` / ``dy_camax``: per-channel maxima of the operands (``_wsdl_camax`` of a
    BatchNorm output / input gradient), ``dy_presplit``: dY as the kernel's fp16 rows (``_wsdl_presplit``) - wsdl_conv2d_wgrad_ex."""
    # maxima / rows that are the operand's OWN attributes are only as good as its version (camax_of): handed over after an
    # in-place edit they are dropped here, and the operand keeps its (re-measured) per-tensor scale
    if x_camax is not None and x_camax is getattr(x, "_wsdl_camax", None) and camax_of(x) is None:
        x_camax = None
    if dy_camax is not None and dy_camax is getattr(dy, "_wsdl_camax", None):
        dy_camax, own_rows = camax_of(dy, presplit=True)
        if dy_presplit is None or dy_presplit is getattr(dy, "_wsdl_presplit", None):
            dy_presplit = own_rows
    if dy_camax is None:
        dy_presplit = None
    if stream is not None and stream != _stream():
        # everything this function would otherwise enqueue on the CURRENT stream (amax passes, densifying copies) must have
        # been resolved by the caller, in front of the wait that orders ``stream`` behind the current one (_wgrad_into)
        split = _wgrad_split(wshape)
        if out is None or (split and (x_amax is None or dy_amax is None)):
            raise WsdlError("conv2d_wgrad(stream=): pass out, x_amax and dy_amax (resolved on the current stream)")
        if _planes(x, "x")[0] is not x or _planes(dy, "dy")[0] is not dy:
            raise WsdlError("conv2d_wgrad(stream=): operands must already be dense planes")
    if x_amax is None:
        x_amax = amax_of(x, _wgrad_split(wshape))
    if dy_amax is None:
        dy_amax = amax_of(dy, _wgrad_split(wshape))
    x, x_bs = _planes(x, "x")
    dy, dy_bs = _planes(dy, "dy")
    B, Cin, H, W = x.shape
    Cout, _, kh, kw = wshape
    geom = (B, Cin, H, W, Cout, kh, kw, stride, pad, dil)
    nbytes = _ws_bytes("wsdl_conv2d_wgrad_workspace", *geom)
    if nbytes == 0:
        raise WsdlError("conv2d_wgrad: bad geometry " + repr(geom))
    ws = workspace(nbytes, x.device, stream)
    if out is None:
        out = torch.empty(wshape, device=x.device, dtype=torch.float32)
        accumulate = False
    check(lib().wsdl_conv2d_wgrad_ex(_p(x), _p(dy), _p(out), *geom, int(accumulate), x_bs, dy_bs, _p(x_amax), _p(dy_amax),
                                     _p(x_camax), _p(dy_camax), _p(dy_presplit), _p(ws), ws.numel(),
                                     _stream() if stream is None else stream))
    return out


def bias_grad(dy, out=None, accumulate=False):
    dy, dy_bs = _planes(dy, "dy")
    B, Cc, H, W = dy.shape
    if out is None:
        out = torch.empty(Cc, device=dy.device, dtype=torch.float32)
        accumulate = False
    check(lib().wsdl_bias_grad(_p(dy), _p(out), B, Cc, H * W, dy_bs, int(accumulate), _stream()))
    return out


def bn_fold(bn_weight, bn_bias, running_mean, running_var, eps):
    Cc = bn_weight.numel()
    scale = torch.empty(Cc, device=bn_weight.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    check(lib().wsdl_bn_fold(_p(_dense(bn_weight)), _p(_dense(bn_bias)), _p(_dense(running_mean)),
                             _p(_dense(running_var)), float(eps), _p(scale), _p(shift), Cc, _stream()))
    return scale, shift


def bn_fold_bias(bn_weight, bn_bias, running_mean, running_var, conv_bias, eps):
    """bn_fold for a convolution that carries a bias in front of its BatchNorm: shift = beta + (bias - rm) * scale."""
    Cc = bn_weight.numel()
    scale = torch.empty(Cc, device=bn_weight.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    check(lib().wsdl_bn_fold_bias(_p(_dense(bn_weight)), _p(_dense(bn_bias)), _p(_dense(running_mean)),
                                  _p(_dense(running_var)), _p(_dense(conv_bias)), float(eps), _p(scale), _p(shift), Cc,
                                  _stream()))
    return scale, shift


# Per-channel maxima from the channel-resident BatchNorm kernels -> per-channel scales of the weight gradients (exact; the range
# guard of the weight gradient for nothing), and the weight gradient's dY operand written pre-split by the BatchNorm backward that
# produces it (no dy_split16 pass).  WSDL_CHAN_AMAX=0 / WSDL_DY_PRESPLIT=0: the round-5 forms (A/B).
CHAN_AMAX = [os.environ.get("WSDL_CHAN_AMAX", "1") != "0"]
DY_PRESPLIT = [os.environ.get("WSDL_DY_PRESPLIT", "1") != "0"]


def _bn_resident(B, Cc, HW, backward):
    key = ("wsdl_bn_channel_resident", (B, Cc, HW, backward))
    r = _size_cache.get(key)
    if r is None:
        r = _size_cache[key] = bool(lib().wsdl_bn_channel_resident(B, Cc, HW, backward))
    return r


# The ReLU mask of a residual layer as bits written by the forward kernel (1/32 of the bytes of y, which the backward would
# otherwise read for it): WSDL_BN_RELU_BITS=0 reads y instead (A/B; same result bit for bit).
BN_RELU_BITS = [os.environ.get("WSDL_BN_RELU_BITS", "1") != "0"]


def bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, residual=None, relu=False, out=None,
                 want_mask=False, mask_if=True, amax_into=None):
    """``want_mask``: returns a fourth value - the ReLU mask as bits (uint8, numel/8 bytes; ``bn_train_bwd(relu_mask=)``),
    or None where the kernels do not write one (no ReLU, H*W not a multiple of 8, ``mask_if`` false)."""
    x = _dense(x, "x")
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
        y_bs = Cc * H * W
    else:
        out, y_bs = _planes(out, "out")
    stats = torch.empty(2, Cc, device=x.device, dtype=torch.float32)      # one allocation for the two saved statistics
    mean, invstd = stats.unbind(0)
    ws = workspace(_ws_bytes("wsdl_bn_workspace", Cc), x.device)
    if residual is not None:
        residual = _dense(residual, "residual")
    # amax_into: a slot shared by several producers (the branches of a concatenation: the maximum over all of them)
    y_amax = (amax_into if amax_into is not None else amax_slot(x.device)) if CONV_ARITH[0] == 1 else None
    mask = None
    if want_mask and mask_if and relu and BN_RELU_BITS[0] and (H * W) % 8 == 0 and y_bs % 4 == 0:
        mask = torch.empty(x.numel() // 8, device=x.device, dtype=torch.uint8)
    # per-channel maxima of the output: the scales of the weight gradient that reads it as its x operand (free in the
    # channel-resident kernel: the channel's workgroup has the maximum anyway)
    camax = None
    if y_amax is not None and CHAN_AMAX[0] and y_bs % 4 == 0 and _bn_resident(B, Cc, H * W, 0):
        camax = torch.empty(Cc, device=x.device, dtype=torch.float32)
    check(lib().wsdl_bn_train_fwd(_p(x), _p(gamma), _p(beta), _p(out), _p(mean), _p(invstd), _p(running_mean),
                                  _p(running_var), float(momentum), float(eps), B, Cc, H * W, _p(residual),
                                  int(relu), y_bs, _p(y_amax), _p(mask), _p(ws), ws.numel(), _p(camax), _stream()))
    if y_amax is not None:
        _publish_amax(out, y_amax)
    if camax is not None:
        _publish_camax(out, camax)
    return (out, mean, invstd, mask) if want_mask else (out, mean, invstd)


def bn_train_bwd(x, dy, y, gamma, mean, invstd, relu, want_dres, dgamma_out=None, dbeta_out=None, accumulate=False,
                 beta=None, relu_mask=None, presplit_bytes=0):
    """``relu``: True with ``y`` = the forward output (mask read from it), or True with ``relu_mask`` = the bits the
    forward wrote (``bn_train_fwd(want_mask=True)``), or True with ``y=None`` and ``beta`` given: the mask is recomputed
    from x (no residual was added in the forward) and y is never touched."""
    x = _dense(x, "x")
    dy, dy_bs = _planes(dy, "dy")
    B, Cc, H, W = x.shape
    y_bs = 0
    mode = 0
    if relu:
        if relu_mask is not None:
            if relu_mask.dtype != torch.uint8 or relu_mask.numel() * 8 != x.numel() or not relu_mask.is_cuda:
                raise WsdlError("bn_train_bwd: relu_mask must be the uint8 bit mask of the forward (numel / 8 bytes)")
            mode = 3
        elif y is None:
            if beta is None:
                raise WsdlError("bn_train_bwd: relu needs the forward output, its bit mask or beta")
            mode = 2
        else:
            mode = 1
            y, y_bs = _planes(y, "y")
    dx = torch.empty_like(x)
    acc = bool(accumulate) and dgamma_out is not None and dbeta_out is not None
    dgamma = dgamma_out if dgamma_out is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = dbeta_out if dbeta_out is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
    dres = torch.empty_like(x) if want_dres else None
    ws = workspace(_ws_bytes("wsdl_bn_workspace", Cc), x.device)
    dx_amax = amax_slot(x.device) if CONV_ARITH[0] == 1 else None
    # ``presplit_bytes`` (wsdl_conv2d_wgrad_presplit_bytes of the convolution whose output gradient this is): dx is also written
    # as the fp16 rows that convolution's weight gradient reads, scaled per channel - dy_split16_kernel does not run for it
    camax = presplit = None
    if dx_amax is not None and CHAN_AMAX[0] and dy_bs % 4 == 0 and y_bs % 4 == 0 and _bn_resident(B, Cc, H * W, 1):
        camax = torch.empty(Cc, device=x.device, dtype=torch.float32)
        if presplit_bytes and DY_PRESPLIT[0] and (B * H * W) % 32 == 0:
            presplit = torch.empty(int(presplit_bytes), device=x.device, dtype=torch.uint8)
    check(lib().wsdl_bn_train_bwd(_p(x), _p(dy), _p(y if mode == 1 else None), _p(gamma),
                                  _p(_dense(beta) if mode == 2 else None), _p(mean), _p(invstd), _p(dx),
                                  _p(dgamma), _p(dbeta), _p(dres), B, Cc, H * W, mode, int(acc), dy_bs, y_bs,
                                  _p(dx_amax), _p(relu_mask if mode == 3 else None), _p(ws), ws.numel(),
                                  _p(camax), _p(presplit), _stream()))
    if dx_amax is not None:
        _publish_amax(dx, dx_amax)
    if camax is not None:
        _publish_camax(dx, camax, presplit)
    dx._wsdl_fresh = True
    if dres is not None:
        dres._wsdl_fresh = True
    return dx, dgamma, dbeta, dres


def _owned(t):
    """May this incoming gradient buffer be accumulated into IN PLACE?  Only buffers the library itself produced for
    exactly this purpose (a BatchNorm-backward ``dres`` / ``dx`` or a dgrad output - marked ``_wsdl_fresh``; the mark
    survives the autograd engine, which either hands the tensor on untouched or sums a fan-out into the first
    arrival, still exclusively its own) and that are not views of something else.  Aliased gradients - the same tensor
    returned twice by an add node, channel slices of a concat's gradient, anything a user hook produced - fall back to
    an out-of-place add."""
    return (t is not None and getattr(t, "_wsdl_fresh", False) and t._base is None and t.is_contiguous()
            and t.dtype == torch.float32 and not t.requires_grad)


def affine_act_bwd(dy, y, scale, relu, want_dconv=True, want_dres=False):
    dy = _dense(dy, "dy")
    B, Cc, H, W = dy.shape
    dconv = torch.empty_like(dy) if want_dconv else None
    dres = torch.empty_like(dy) if want_dres else None
    amax = amax_slot(dy.device) if (want_dconv and CONV_ARITH[0] == 1) else None
    check(lib().wsdl_affine_act_bwd(_p(dy), _p(_dense(y) if relu else None), _p(scale), _p(dconv), _p(dres), B, Cc,
                                    H * W, int(relu), _p(amax), _stream()))
    if amax is not None:
        _publish_amax(dconv, amax)
    return dconv, dres


# ------------------------------------------------------------------------------------------ autograd
# Weight gradients are only consumed by the optimiser step, so they run on a side HIP stream: the MFMA-bound
# wgrad kernels overlap the HBM-bound BatchNorm backward / gradient-reduce kernels of the main chain.
OVERLAP_WGRAD = [True]
WGRAD_AFTER_DGRAD = [False]     # measured: 21.2 ms/step against 20.9 with the weight gradient enqueued first (profiles/r02_notes.md)
LAST_WGRAD_ON_MAIN = [os.environ.get("WSDL_LAST_WGRAD_ON_MAIN", "1") != "0"]   # the stem's weight gradient: see _wgrad_into
_side_streams = {}


def side_stream(device):
    if device.index is None:
        device = _norm_device(device)
    st = _side_streams.get(device)
    if st is None:
        st = _side_streams[device] = torch.cuda.Stream(device=device)
    return st


def join_side_stream(device):
    """Make the current stream wait for everything queued on the side stream (before the optimiser step / a
    gradient all-reduce reads the flat gradient buffer)."""
    st = _side_streams.get(_norm_device(device))
    if st is not None:
        stream_wait(raw_stream(device), st)


def _wgrad_into(param, x, dconv, wshape, stride, pad, dil, sink, x_amax=None, last=False, x_camax=None):
    """d(param) = wgrad(x, dconv) written straight into param.grad (a slice of the flat gradient buffer).
    ``last``: no input gradient follows (the network's first layer): nothing else is left for the main stream, so the
    kernel runs there, beside whatever the side stream still has queued, instead of behind it."""
    accumulate = not sink.take_fresh(param)
    split = _wgrad_split(wshape)
    x_amax = x_amax if x_amax is not None else amax_of(x, split)       # resolved on the MAIN stream (may launch a pass)
    dy_amax = amax_of(dconv, split)
    # per-channel maxima / pre-split rows travel as attributes of the tensors their producers returned
    dy_camax, dy_presplit = camax_of(dconv, presplit=True) if split else (None, None)
    if not split:
        x_camax = None
    elif x_camax is None:
        x_camax = camax_of(x)
    if x_camax is not None and x_camax.numel() != wshape[1]:
        x_camax = None                  # (a channel slice / concatenation of the tensor that carried it)
    if OVERLAP_WGRAD[0] and not (last and LAST_WGRAD_ON_MAIN[0]):
        # a densifying copy (never needed by the training step's own tensors) would be enqueued on the CURRENT stream: make it
        # happen before the side stream's wait, not inside conv2d_wgrad behind it
        x, dconv = _planes(x, "x")[0], _planes(dconv, "dy")[0]
        side = side_stream(x.device)
        hside = side.cuda_stream
        stream_wait(hside, _stream())               # dconv / x (and the zero_grad memset) are ready
        # launched ON the side stream by handle: torch's current stream stays the main one
        conv2d_wgrad(x, dconv, wshape, stride, pad, dil, out=param.grad, accumulate=accumulate, x_amax=x_amax,
                     dy_amax=dy_amax, stream=hside, x_camax=x_camax, dy_camax=dy_camax,
                     dy_presplit=dy_presplit)
        for t in (x_camax, dy_camax, dy_presplit):
            if t is not None:
                t.record_stream(side)
        x.record_stream(side)                       # keep the caching allocator from recycling them early
        dconv.record_stream(side)
    else:
        conv2d_wgrad(x, dconv, wshape, stride, pad, dil, out=param.grad, accumulate=accumulate, x_amax=x_amax,
                     dy_amax=dy_amax, x_camax=x_camax, dy_camax=dy_camax, dy_presplit=dy_presplit)
    sink.grad_ready(param)


def _sink_of(param):
    """Parameters owned by a FlatAdam carry ``_wsdl_grad_sink``: their gradient is written by the kernels
    straight into the optimiser's flat gradient buffer (no autograd accumulation pass, no extra add)."""
    sink = getattr(param, "_wsdl_grad_sink", None)
    if sink is None or param.grad is None or not param.grad.is_cuda:
        return None
    return sink


def _alias(t):
    """A tensor over the same memory that autograd knows nothing about (not a view of ``t`` in its books): what a kernel
    that writes into a slice of somebody else's buffer returns as its output."""
    return torch.empty(0, device=t.device, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset(), t.shape, t.stride())


class IdentityLink:
    """Shared by the two ``conv_bn_act`` calls that open and close an identity bottleneck (train mode).  The gradient of the
    block's input through the identity branch is [y > 0] * dy (dy: the gradient of the block's output, y its final ReLU).
    Routed through autograd it is a tensor the last BatchNorm backward writes (``dres``) and the first convolution's dgrad
    epilogue reads back.  With a link the last node leaves (dy, the ReLU's bits) here, returns no gradient for the residual
    input, and the first node - whose backward always runs later: its output's gradient depends on the rest of the block -
    adds [bits] * dy inside its dgrad epilogue, in dy's own buffer: one tensor write and one allocation less per block.
    Only when dy is a buffer the library owns (``_owned``); otherwise the ``dres`` path runs as before.  WSDL_IDENTITY_LINK=0
    switches it off (A/B; same result bit for bit)."""
    __slots__ = ("pending", "projection")

    def __init__(self, projection=False):
        # projection: the block's shortcut is a convolution + BatchNorm (the first block of a layer).  Then the link joins the
        # block's LAST node and that shortcut node: the last node hands the shortcut dy itself as "gradient" (an alias: no
        # tensor written) and the bits here; the shortcut's BatchNorm backward applies them (relu = 3) to what it reads.
        self.pending = None
        self.projection = projection


IDENTITY_LINK = [os.environ.get("WSDL_IDENTITY_LINK", "1") != "0"]


class _ConvBNAct(torch.autograd.Function):
    """Train-mode conv -> BatchNorm(batch statistics) -> (+residual) -> ReLU as one autograd node."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, running_mean, running_var, stride, pad, dil, relu,
                momentum, eps, cache=None, passthrough=False, link=None, out_holder=None):
        # out_holder ([view into a larger buffer, shared amax slot] - a list, so that autograd does not see the tensors): the
        # BatchNorm kernel writes its output straight into a channel slice of a concatenation buffer (ASPP) - see concat_into
        # link (IdentityLink, shared by the first and the last node of an identity bottleneck): the last node's backward
        # does not write the masked gradient of the identity branch; it leaves (dy, mask bits) in the link and the first
        # node's dgrad epilogue adds [mask] * dy into dy's buffer - see IdentityLink
        ctx.link = link
        if link is not None:
            ctx.set_materialize_grads(False)
        # passthrough: also hand x back as a second output (the identity branch of a bottleneck).  The gradient that
        # arrives for it is then added inside the dgrad kernel's epilogue instead of by a separate autograd add.
        wf, wd = _cached_prep(cache, weight, x.requires_grad)
        x_amax = amax_of(x, _split_kc(x.shape[1], weight.shape[2] * weight.shape[3]) or _wgrad_split(weight.shape))
        conv = conv2d_fwd(x, wf, weight.shape, stride, pad, dil, x_amax=x_amax)
        y, mean, invstd, rbits = bn_train_fwd(conv, _dense(gamma), _dense(beta), running_mean, running_var, momentum, eps,
                                              residual, relu, out=_alias(out_holder[0]) if out_holder else None,
                                              want_mask=True, mask_if=bool(relu) and residual is not None,
                                              amax_into=out_holder[1] if out_holder else None)
        ctx.cfg = (stride, pad, dil, relu, tuple(weight.shape), tuple(x.shape), residual is not None)
        ctx.params = (weight, gamma, beta)
        ctx.x_amax = x_amax              # saved tensors come back as new Python objects: keep the scalar explicitly
        ctx.x_camax = camax_of(x)     # ... and the per-channel maxima its producer published
        # the ReLU mask is recomputed from the conv output in the backward unless a residual was added: then the forward
        # kernel wrote it as bits (or, where it cannot - H*W not a multiple of 8 - y is kept and read)
        ctx.save_for_backward(x, conv, y if (relu and residual is not None and rbits is None) else None, gamma, mean, invstd,
                              wd, beta if relu else None, rbits)
        if passthrough:
            xv = x.view_as(x)
            if x_amax is not None:
                _publish_amax(xv, x_amax)
            if ctx.x_camax is not None:
                _publish_camax(xv, ctx.x_camax)
            return y, xv
        return y

    @staticmethod
    def backward(ctx, dy, dxres=None):
        x, conv, y, gamma, mean, invstd, wd, beta_s, rbits = ctx.saved_tensors
        stride, pad, dil, relu, wshape, xshape, has_res = ctx.cfg
        pw, pg, pb = ctx.params
        need_res = has_res and ctx.needs_input_grad[4]
        link = ctx.link
        if dy is None:
            raise WsdlError("conv -> BatchNorm node: no gradient arrived for its output")
        alias_dres = False
        if (link is not None and need_res and rbits is not None and IDENTITY_LINK[0] and tuple(dy.shape) == tuple(conv.shape)
                and dy.is_contiguous()):
            if link.projection:
                link.pending = (dy, rbits)   # consumed by the shortcut's node, which receives dy itself as its gradient
                need_res, alias_dres = False, True
            elif _owned(dy):
                link.pending = (dy, rbits)   # consumed by the block's first node (its backward runs after this one)
                need_res = False
        # the shortcut node of a projection block: its "gradient" is the block output's dy, to be masked by the bits
        shortcut_bits = None
        if link is not None and link.projection and not has_res:
            if link.pending is not None:
                src, shortcut_bits = link.pending
                link.pending = None
                if src.data_ptr() != dy.data_ptr() or tuple(src.shape) != tuple(dy.shape):
                    raise WsdlError("projection shortcut: the gradient that arrived is not the block output's (autograd "
                                    "copied or summed it) - set WSDL_IDENTITY_LINK=0")
        if shortcut_bits is not None:
            relu_b, y_b, beta_b, bits_b = True, None, None, shortcut_bits      # dy' = [bits] * dy, then this node's BatchNorm
        else:
            relu_b, y_b, beta_b, bits_b = relu, y, beta_s, rbits
        sg = _sink_of(pg) if (ctx.needs_input_grad[2] and ctx.needs_input_grad[3] and _sink_of(pg) is _sink_of(pb)) else None
        # the weight gradient's dY operand, written pre-split by the BatchNorm backward where that launch reads it so
        psb = wgrad_presplit_bytes(xshape, wshape, stride, pad, dil) if (ctx.needs_input_grad[1] and _sink_of(pw) is not None) else 0
        if sg is not None:
            fresh = sg.take_fresh(pg) & sg.take_fresh(pb)
            dconv, _, _, dres = bn_train_bwd(conv, dy, y_b, _dense(gamma), mean, invstd, relu_b, need_res,
                                             pg.grad, pb.grad, accumulate=not fresh, beta=beta_b, relu_mask=bits_b,
                                             presplit_bytes=psb)
            dgamma = dbeta = None
            sg.grad_ready(pg)
            sg.grad_ready(pb)
        else:
            dconv, dgamma, dbeta, dres = bn_train_bwd(conv, dy, y_b, _dense(gamma), mean, invstd, relu_b, need_res, beta=beta_b,
                                                      relu_mask=bits_b)
        if alias_dres:
            dres = dy
        pend = None
        if link is not None and not link.projection and link.pending is not None and not has_res:
            pend, link.pending = link.pending, None

        def input_grad():
            dx = None
            if ctx.needs_input_grad[0]:
                if wd is None:
                    raise WsdlError("conv backward: dgrad weights were not prepared")
                into, bits = None, None
                if pend is not None and tuple(pend[0].shape) == tuple(xshape):
                    into, bits = pend       # the block output's gradient + the final ReLU's bits: dx = dgrad(...) + [bits] * it
                elif _owned(dxres) and tuple(dxres.shape) == tuple(xshape):
                    into = dxres        # the identity branch's gradient (a fresh BN-backward output): dx = dgrad(...) + it
                dx = conv2d_dgrad(dconv, wd, wshape, xshape, stride, pad, dil, accumulate_into=into, acc_mask=bits)
                if into is None and dxres is not None:
                    dx = dx + dxres
                elif bits is not None and dxres is not None:
                    dx = dx + dxres          # (does not happen: the link replaces the gradient of the passthrough output)
            elif dxres is not None:
                dx = dxres
            return dx

        # Order of the two MFMA-bound kernels.  The weight gradient runs on the side stream behind everything enqueued on
        # the main stream so far.  WGRAD_AFTER_DGRAD: enqueue the input gradient FIRST, so the weight gradient starts when
        # it has finished and runs beside the NEXT layer's BatchNorm backward (HBM-bound) instead of beside this layer's
        # input gradient (two MFMA-bound kernels sharing one power budget gain nothing from overlapping).
        dx = input_grad() if WGRAD_AFTER_DGRAD[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            sw = _sink_of(pw)
            if sw is not None:
                _wgrad_into(pw, x, dconv, wshape, stride, pad, dil, sw, ctx.x_amax, last=not ctx.needs_input_grad[0],
                            x_camax=ctx.x_camax)
            else:
                dw = conv2d_wgrad(x, dconv, wshape, stride, pad, dil, x_amax=ctx.x_amax)
        if not WGRAD_AFTER_DGRAD[0]:
            dx = input_grad()
        return (dx, dw, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None,
                dres, None, None, None, None, None, None, None, None, None, None, None, None)


ASPP_MULTI = [os.environ.get("WSDL_ASPP_MULTI", "1") != "0"]     # A/B: 0 = the branches as a chain of conv -> BatchNorm nodes
ASPP_GROUP_FWD = [os.environ.get("WSDL_ASPP_GROUP_FWD", "1") != "0"]   # A/B: 0 = the branches' forward convolutions one launch each


class _ConvBNBranches(torch.autograd.Function):
    """n train-mode conv -> BatchNorm -> ReLU branches over ONE input (the 1x1 and the three dilated 3x3 branches of ASPP), each
    writing its output into its channel slice of the concatenation buffer.  What it does differently from n chained
    ``_ConvBNAct`` nodes is the input gradient: ONE launch that accumulates all branches' taps per output tile
    (``conv2d_dgrad_multi``) instead of n launches that each read the running sum back and write it again.
    Arguments: x, momentum, eps, branches = [(stride-1 padding, dilation, cache, out_holder)], then per branch
    weight, gamma, beta, running_mean, running_var.  Returns y_0 .. y_{n-1}, x' (x routed through the node: the gradient
    arriving for it - the pooling branch's - is the launch's ``accumulate_into``)."""

    @staticmethod
    def forward(ctx, x, momentum, eps, branches, *tensors):
        n = len(branches)
        params = [tensors[5 * i:5 * i + 5] for i in range(n)]
        taps = max(w.shape[2] * w.shape[3] for (w, *_r) in params)
        x_amax = amax_of(x, _split_kc(x.shape[1], taps) or any(_wgrad_split(w.shape) for (w, *_r) in params))
        saved, outs, wshapes = [x], [], []
        preps = [_cached_prep(cache, w, x.requires_grad) for (_pad, _dil, cache, _h), (w, *_r) in zip(branches, params)]
        convs = None
        if ASPP_GROUP_FWD[0] and fwd_group_ok(n, tuple(x.shape), params[0][0].shape[0]):
            convs = conv2d_fwd_group(x, [pr[0] for pr in preps], [tuple(w.shape) for (w, *_r) in params],
                                     [b[1] for b in branches], x_amax=x_amax)
        for i, ((pad, dil, cache, holder), (w, gamma, beta, rm, rv)) in enumerate(zip(branches, params)):
            wf, wd = preps[i]
            conv = convs[i] if convs is not None else conv2d_fwd(x, wf, w.shape, 1, pad, dil, x_amax=x_amax)
            y, mean, invstd, _bits = bn_train_fwd(conv, _dense(gamma), _dense(beta), rm, rv, momentum, eps, None, True,
                                                  out=_alias(holder[0]), want_mask=True, mask_if=False, amax_into=holder[1])
            saved += [conv, gamma, mean, invstd, wd, beta]
            outs.append(y)
            wshapes.append(tuple(w.shape))
        ctx.cfg = ([(b[0], b[1]) for b in branches], wshapes, tuple(x.shape))
        ctx.params = [(w, g, b) for (w, g, b, _rm, _rv) in params]
        ctx.x_amax = x_amax
        ctx.x_camax = camax_of(x)
        ctx.save_for_backward(*saved)
        xv = x.view_as(x)
        if x_amax is not None:
            _publish_amax(xv, x_amax)
        if ctx.x_camax is not None:
            _publish_camax(xv, ctx.x_camax)
        return (*outs, xv)

    @staticmethod
    def backward(ctx, *grads):
        geo, wshapes, xshape = ctx.cfg
        n = len(geo)
        dys, dxres = grads[:n], grads[n]
        saved = ctx.saved_tensors
        x = saved[0]
        dconvs, wds = [], []
        for i in range(n):
            conv, gamma, mean, invstd, wd, beta = saved[1 + 6 * i:7 + 6 * i]
            pw, pg, pb = ctx.params[i]
            if dys[i] is None:
                raise WsdlError("conv -> BatchNorm branches: no gradient arrived for branch %d" % i)
            sg = _sink_of(pg)
            if sg is None or sg is not _sink_of(pb) or _sink_of(pw) is None:
                raise WsdlError("conv -> BatchNorm branches: the parameters must be owned by a FlatAdam (gradient sinks)")
            fresh = sg.take_fresh(pg) & sg.take_fresh(pb)
            pad, dil = geo[i]
            dconv, _, _, _ = bn_train_bwd(conv, dys[i], None, _dense(gamma), mean, invstd, True, False, pg.grad, pb.grad,
                                          accumulate=not fresh, beta=beta,
                                          presplit_bytes=wgrad_presplit_bytes(xshape, wshapes[i], 1, pad, dil))
            sg.grad_ready(pg)
            sg.grad_ready(pb)
            _wgrad_into(pw, x, dconv, wshapes[i], 1, pad, dil, _sink_of(pw), ctx.x_amax, x_camax=ctx.x_camax)
            dconvs.append(dconv)
            wds.append(wd)
        dx = None
        if ctx.needs_input_grad[0]:
            into = dxres if (_owned(dxres) and tuple(dxres.shape) == tuple(xshape)) else None
            # the source that decides the column bands first: the smallest dilation among the 3x3 branches
            order = sorted(range(n), key=lambda i: (wshapes[i][2] == 1, geo[i][1]))
            dx = conv2d_dgrad_multi([dconvs[i] for i in order], [wds[i] for i in order], [wshapes[i] for i in order],
                                    [geo[i][1] for i in order], xshape, accumulate_into=into)
            if into is None and dxres is not None:
                dx = dx + dxres
        elif dxres is not None:
            dx = dxres
        return (dx, None, None, None) + (None,) * (5 * n)


def conv_bn_branches(x, branches, momentum, eps):
    """``branches``: [(conv module-like with .weight/.padding/.dilation and a cache dict, bn module-like, out_holder)] - see
    _ConvBNBranches; the caller (ASPP) has checked ``dgrad_multi_ok`` and train mode."""
    geo, tensors = [], []
    for conv, bn, holder in branches:
        geo.append((conv.padding, conv.dilation, conv.__dict__.setdefault("_wsdl_cache", {}), holder))
        tensors += [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    bump_stats_epoch()
    return _ConvBNBranches.apply(x, momentum, eps, geo, *tensors)


class _ConvAffineAct(torch.autograd.Function):
    """y = act(scale*conv(x,w) + shift + residual): eval-mode (folded) BN, conv bias, Linear."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, residual, stride, pad, dil, relu, shift_is_param, cache=None):
        need_dx = x.requires_grad
        wf, wd = _cached_prep(cache, weight, need_dx)
        # a folded-BatchNorm convolution (eval mode) feeds the next convolution directly: its epilogue publishes the amax
        y = conv2d_fwd(x, wf, weight.shape, stride, pad, dil, scale, shift, residual, relu,
                       want_amax=bool(relu) or scale is not None)
        ctx.cfg = (stride, pad, dil, relu, tuple(weight.shape), tuple(x.shape), residual is not None, shift_is_param)
        ctx.params = (weight, shift if shift_is_param else None)
        need_w = weight.requires_grad
        ctx.save_for_backward(x if need_w else None, y if relu else None, scale, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, scale, wd = ctx.saved_tensors
        stride, pad, dil, relu, wshape, xshape, has_res, shift_is_param = ctx.cfg
        need_res = has_res and ctx.needs_input_grad[4]
        dyc = _dense(dy, "dy")
        if relu or scale is not None or need_res:
            dconv, dres = affine_act_bwd(dyc, y, scale, relu, True, need_res)
            if need_res and not relu:
                dres = dyc
        else:
            dconv, dres = dyc, None
        pw, pbias = ctx.params
        dw = None
        if ctx.needs_input_grad[1]:
            sw = _sink_of(pw)
            if sw is not None and tuple(pw.grad.shape) == tuple(wshape):
                _wgrad_into(pw, x, dconv, wshape, stride, pad, dil, sw)
            else:
                dw = conv2d_wgrad(x, dconv, wshape, stride, pad, dil)
        dshift = None
        if ctx.needs_input_grad[3] and shift_is_param:
            # with scale None the shift is a plain bias: d/dshift = sum of the masked upstream gradient
            sb = _sink_of(pbias)
            if sb is not None:
                bias_grad(dconv, out=pbias.grad, accumulate=not sb.take_fresh(pbias))
                sb.grad_ready(pbias)
            else:
                dshift = bias_grad(dconv)
        dx = conv2d_dgrad(dconv, wd, wshape, xshape, stride, pad, dil) if ctx.needs_input_grad[0] else None
        return dx, dw, None, dshift, dres, None, None, None, None, None, None


class _BNTrain(torch.autograd.Function):
    """Stand-alone train-mode BatchNorm2d (batch statistics, running-statistics update): the same two kernels the
    fused conv -> BN node runs, without the convolution."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps):
        x = _dense(x, "x")
        y, mean, invstd = bn_train_fwd(x, _dense(gamma), _dense(beta), running_mean, running_var, momentum, eps)
        ctx.save_for_backward(x, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd = ctx.saved_tensors
        dx, dgamma, dbeta, _ = bn_train_bwd(x, dy, None, _dense(gamma), mean, invstd, False, False)
        return dx, dgamma, dbeta, None, None, None, None


class _AffineAct(torch.autograd.Function):
    """y = act(scale[c]*x + shift[c]) on (B,C,H,W) [or (B,C)]: stand-alone eval-mode BatchNorm2d / ReLU."""

    @staticmethod
    def forward(ctx, x, scale, shift, relu):
        x = _dense(x, "x")
        B, Cc = (x.shape[0], x.shape[1]) if x.dim() >= 2 else (1, 1)
        HW = x.numel() // max(B * Cc, 1)
        y = torch.empty_like(x)
        check(lib().wsdl_affine_act_fwd(_p(x), _p(scale), _p(shift), _p(y), B, Cc, HW, int(relu), _stream()))
        ctx.relu, ctx.geom = relu, (B, Cc, HW)
        ctx.save_for_backward(y if relu else None, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, scale = ctx.saved_tensors
        B, Cc, HW = ctx.geom
        dy = _dense(dy, "dy")
        if not ctx.relu and scale is None:
            return dy, None, None, None
        dx = torch.empty_like(dy)
        check(lib().wsdl_affine_act_bwd(_p(dy), _p(y), _p(scale), _p(dx), _vp(0), B, Cc, HW, int(ctx.relu), _vp(0), _stream()))
        return dx, None, None, None


def batch_norm(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, training=True):
    """Stand-alone nn.BatchNorm2d.forward.  Eval mode folds the running statistics; like the fused eval path it
    treats gamma / beta as constants (the frozen classifier is the only eval-mode user of the reference)."""
    if training:
        bump_stats_epoch()
        return _BNTrain.apply(x, gamma, beta, running_mean, running_var, momentum, eps)
    scale, shift = bn_fold(gamma.detach(), beta.detach(), running_mean, running_var, eps)
    return _AffineAct.apply(x, scale, shift, False)


def relu(x):
    return _AffineAct.apply(x, None, None, True)


def check_group_norm_options(num_groups, num_channels=None, eps=1e-5, name="group_norm"):
    """Host-side validation of GroupNorm's options, before any device call: WsdlError unless ``num_groups`` is an int >= 1 that
    divides ``num_channels`` (an int >= 1, if given) and ``eps`` is a finite number >= 0."""
    if isinstance(num_groups, bool) or not isinstance(num_groups, int) or num_groups < 1:
        raise WsdlError(f"{name}: num_groups {num_groups!r} must be an int >= 1")
    if num_channels is not None:
        if isinstance(num_channels, bool) or not isinstance(num_channels, int) or num_channels < 1:
            raise WsdlError(f"{name}: num_channels {num_channels!r} must be an int >= 1")
        if num_channels % num_groups:
            raise WsdlError(f"{name}: num_groups {num_groups} does not divide the {num_channels} channels")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 <= float(eps) < float("inf")):
        raise WsdlError(f"{name}: eps {eps!r} must be a finite number >= 0")


def _group_norm_ws(B, Cc, HW, G, device):
    nbytes = _ws_bytes("wsdl_group_norm_workspace", B, Cc, HW, G)
    if nbytes == 0:
        raise WsdlError(f"group_norm: bad geometry B={B} C={Cc} HW={HW} num_groups={G} (at most 2^31 - 1 elements)")
    return workspace(nbytes, device)


def group_norm_bwd(x, dy, y, gamma, stats, num_groups, relu, dx=None, dgamma=None, dbeta=None, accumulate=False):
    """wsdl_group_norm_bwd on dense tensors: writes the gradients whose buffers are given (``dx`` like x, ``dgamma`` / ``dbeta``
    (C,) float32; with ``accumulate`` the two parameter gradients are added to) and launches nothing for the others.  ``stats``:
    the (2, B G) float64 mean / rstd the forward saved; ``y``: the forward output, read only under ``relu``."""
    B, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // (B * Cc)
    ws = _group_norm_ws(B, Cc, HW, num_groups, x.device)
    check(lib().wsdl_group_norm_bwd(_p(x), _p(dy), _p(y if relu else None), _p(gamma), _p(stats[0]), _p(stats[1]), _p(dx), _p(dgamma),
                                    _p(dbeta), B, Cc, HW, num_groups, int(relu), int(accumulate), _p(ws), ws.numel(), _stream()))


def _grad_slot(param, wanted, Cc):
    """(buffer, accumulate, sink) for a (C,) parameter gradient: the parameter's slice of a flat optimiser's gradient buffer
    (``_sink_of``; take_fresh -> accumulate, as the convolution's bias) or a new tensor to hand back to autograd."""
    if not wanted:
        return None, False, None
    sink = _sink_of(param)
    if sink is not None and tuple(param.grad.shape) == (Cc,) and param.grad.is_contiguous() and param.grad.dtype == torch.float32:
        return param.grad, not sink.take_fresh(param), sink
    return torch.empty(Cc, device=param.device, dtype=torch.float32), False, None


class _GroupNorm(torch.autograd.Function):
    """wsdl_group_norm_fwd / _bwd: three launches each way (two in the backward when x needs no gradient).  The statistics are
    saved in double; the backward launches for the needed gradients only and writes those of parameters a flat optimiser owns
    straight into ``p.grad``."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, relu):
        x = _dense(x, "group_norm: x")
        B, Cc = x.shape[0], x.shape[1]
        HW = x.numel() // (B * Cc)
        gamma = None if weight is None else _dense(weight.detach(), "group_norm: weight")
        beta = None if bias is None else _dense(bias.detach(), "group_norm: bias")
        y = torch.empty_like(x)
        stats = torch.empty(2, B * num_groups, device=x.device, dtype=torch.float64)      # mean, rstd
        ws = _group_norm_ws(B, Cc, HW, num_groups, x.device)
        check(lib().wsdl_group_norm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats[0]), _p(stats[1]), B, Cc, HW, num_groups, eps,
                                        int(relu), _p(ws), ws.numel(), _stream()))
        ctx.cfg = (num_groups, relu)
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, gamma, stats, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats, y = ctx.saved_tensors
        num_groups, relu = ctx.cfg
        pw, pb = ctx.params
        Cc = x.shape[1]
        dy = _dense(dy, "group_norm: upstream gradient")
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dg, acc_g, sink_g = _grad_slot(pw, pw is not None and ctx.needs_input_grad[1], Cc)
        db, acc_b, sink_b = _grad_slot(pb, pb is not None and ctx.needs_input_grad[2], Cc)
        if dg is not None and db is not None and acc_g != acc_b:
            # one of the two is added to and the other stored (a parameter shared with another layer): a call each
            group_norm_bwd(x, dy, y, gamma, stats, num_groups, relu, dx=dx, dgamma=dg, accumulate=acc_g)
            group_norm_bwd(x, dy, y, gamma, stats, num_groups, relu, dbeta=db, accumulate=acc_b)
        elif dx is not None or dg is not None or db is not None:
            group_norm_bwd(x, dy, y, gamma, stats, num_groups, relu, dx=dx, dgamma=dg, dbeta=db, accumulate=acc_g or acc_b)
        if sink_g is not None:
            sink_g.grad_ready(pw)
            dg = None
        if sink_b is not None:
            sink_b.grad_ready(pb)
            db = None
        return dx, dg, db, None, None, None


def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, relu=False):
    """``torch.nn.functional.group_norm`` for a float32 device tensor (B, C, *) with at least two dimensions, optionally followed
    by a fused ReLU: over each group of ``C / num_groups`` channels of an image, ``y = (x - mean) / sqrt(var + eps) * weight[c] +
    bias[c]`` with the biased variance.  Train and eval are the same function.  A group of one element is accepted (``y = bias``,
    zero gradient to x).  Statistics and every backward sum in double, the variance from a shifted second moment, partials
    combined in a fixed order without atomics: bitwise reproducible, no host read - a launch plan can hold the call and its
    backward.  Differentiable in ``x``, ``weight`` and ``bias``; the gradients of parameters owned by a flat optimiser go
    straight into ``p.grad``.  Non-dense inputs are copied first."""
    check_group_norm_options(num_groups, eps=eps)
    if not torch.is_tensor(x) or x.dim() < 2:
        raise WsdlError("group_norm: x must be a (B, C, *) tensor with at least two dimensions")
    check_group_norm_options(num_groups, int(x.shape[1]), eps)
    _req(x, "group_norm: x")
    if x.numel() == 0:
        raise WsdlError(f"group_norm: x {tuple(x.shape)} has an empty dimension")
    for t, name in ((weight, "weight"), (bias, "bias")):
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (x.shape[1],):
            raise WsdlError(f"group_norm: {name} must be a ({x.shape[1]},) tensor")
        _req(t, f"group_norm: {name}")
        if t.device != x.device:
            raise WsdlError(f"group_norm: {name} is on {t.device}, x on {x.device}")
    return _GroupNorm.apply(x, weight, bias, num_groups, float(eps), bool(relu))


class _MaxPool3x3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dense(x, "x")
        B, Cc, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(B, Cc, OH, OW, device=x.device, dtype=torch.float32)
        am = torch.empty(B, Cc, OH, OW, device=x.device, dtype=torch.uint8)
        check(lib().wsdl_maxpool3x3s2_fwd(_p(x), _p(y), _p(am), B * Cc, H, W, _stream()))
        ctx.save_for_backward(am)
        ctx.xshape = tuple(x.shape)
        if getattr(x, "_wsdl_amax", None) is not None and getattr(x, "_wsdl_amax_version", x._version) == x._version:
            _publish_amax(y, x._wsdl_amax)       # max over windows of x: the input's bound holds (x >= 0 after ReLU or not)
        return y

    @staticmethod
    def backward(ctx, dy):
        (am,) = ctx.saved_tensors
        B, Cc, H, W = ctx.xshape
        dx = torch.empty(ctx.xshape, device=dy.device, dtype=torch.float32)
        check(lib().wsdl_maxpool3x3s2_bwd(_p(_dense(dy)), _p(am), _p(dx), B * Cc, H, W, _stream()))
        return dx


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dense(x, "x")
        B, Cc, H, W = x.shape
        y = torch.empty(B, Cc, 1, 1, device=x.device, dtype=torch.float32)
        check(lib().wsdl_global_avgpool_fwd(_p(x), _p(y), B * Cc, H * W, _stream()))
        ctx.xshape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Cc, H, W = ctx.xshape
        dx = torch.empty(ctx.xshape, device=dy.device, dtype=torch.float32)
        check(lib().wsdl_global_avgpool_bwd(_p(_dense(dy)), _p(dx), B * Cc, H * W, 0, _stream()))
        dx._wsdl_fresh = True       # ASPP: the pooling branch's input gradient is summed into by the conv branches' dgrads
        return dx


class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        x = _dense(x, "x")
        B, Cc, h, w = x.shape
        y = torch.empty(B, Cc, H, W, device=x.device, dtype=torch.float32)
        check(lib().wsdl_bilinear_fwd(_p(x), _p(y), B, Cc, h, w, H, W, 0, _stream()))
        ctx.shape = (B, Cc, h, w, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Cc, h, w, H, W = ctx.shape
        dy, dy_bs = _planes(dy, "dy")
        dx = torch.empty(B, Cc, h, w, device=dy.device, dtype=torch.float32)
        check(lib().wsdl_bilinear_bwd(_p(dy), _p(dx), B, Cc, h, w, H, W, dy_bs, _stream()))
        return dx, None, None


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, mask, counter=None):
        x = _dense(x, "x")
        y = torch.empty_like(x)
        gen = mask is None
        if gen:
            mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        else:
            mask = _req(mask, "dropout mask", torch.uint8).contiguous()
        check(lib().wsdl_dropout_fwd(_p(x), _p(y), _p(mask), x.numel(), float(p), int(seed), int(gen), _p(counter),
                                     _stream()))
        if counter is not None and gen:
            add_int(counter, 1)         # on the stream, behind the kernel that read it (a node of a captured graph / a plan too)
        ctx.save_for_backward(mask)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = _dense(dy, "dy")
        dx = torch.empty_like(dy)
        check(lib().wsdl_dropout_bwd(_p(dy), _p(mask), _p(dx), dy.numel(), ctx.p, _stream()))
        return dx, None, None, None, None


class _ConcatChannels(torch.autograd.Function):
    """torch.cat(dim=1) with plane copies; backward hands out zero-copy channel slices."""

    @staticmethod
    def forward(ctx, *xs):
        B, _, H, W = xs[0].shape
        Cs = [int(t.shape[1]) for t in xs]
        out = torch.empty(B, sum(Cs), H, W, device=xs[0].device, dtype=torch.float32)
        off, tot = 0, sum(Cs) * H * W
        for t, c in zip(xs, Cs):
            t = _dense(t, "cat input")
            dst = out[:, off:off + c]
            check(lib().wsdl_copy_planes(_p(t), _p(dst), B, c, H * W, 0, tot, _stream()))
            off += c
        ctx.Cs = Cs
        return out

    @staticmethod
    def backward(ctx, dy):
        outs, off = [], 0
        for c in ctx.Cs:
            outs.append(dy[:, off:off + c])
            off += c
        return tuple(outs)


class _ConcatInto(torch.autograd.Function):
    """torch.cat(dim=1) into a buffer some of whose channel slices the producers have already written (``out_holder`` of
    ``conv_bn_act``): only the other inputs are copied.  ``holder`` = [buffer, shared amax slot or None]."""

    @staticmethod
    def forward(ctx, holder, *xs):
        base, slot = holder
        B, Ctot, H, W = base.shape
        Cs = [int(t.shape[1]) for t in xs]
        if sum(Cs) != Ctot:
            raise WsdlError("concat_into: channel counts do not add up to the buffer's")
        off, tot = 0, Ctot * H * W
        for t, c in zip(xs, Cs):
            dst = base[:, off:off + c]
            in_place = (t.data_ptr() == dst.data_ptr() and tuple(t.shape) == tuple(dst.shape) and t.stride() == dst.stride())
            if not in_place:
                t = _dense(t, "cat input")
                check(lib().wsdl_copy_planes(_p(t), _p(dst), B, c, H * W, 0, tot, _stream()))
                if slot is not None:      # this input's maximum joins the slot the in-place producers published into
                    check(lib().wsdl_amax(_p(t), B, c * H * W, c * H * W, _p(slot), 0, _stream()))
            off += c
        ctx.Cs = Cs
        out = _alias(base)
        if slot is not None:
            _publish_amax(out, slot)
        return out

    @staticmethod
    def backward(ctx, dy):
        outs, off = [None], 0
        for c in ctx.Cs:
            outs.append(dy[:, off:off + c])
            off += c
        return tuple(outs)


def concat_into(base, slot, xs):
    return _ConcatInto.apply([base, slot], *xs)


class _AddAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, relu):
        a, b = _dense(a, "a"), _dense(b, "b")
        y = torch.empty_like(a)
        check(lib().wsdl_add(_p(a), _p(b), _p(y), a.numel(), int(relu), _stream()))
        ctx.relu = relu
        ctx.save_for_backward(y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if ctx.relu:
            dy4 = dy if dy.dim() == 4 else dy.reshape(dy.shape[0], -1, 1, 1)
            y4 = y.reshape(dy4.shape)
            g, _ = affine_act_bwd(dy4, y4, None, True, True, False)
            g = g.reshape(dy.shape)
        else:
            g = dy
        return g, g, None


class _SoftmaxCE(torch.autograd.Function):
    """nn.CrossEntropyLoss() on (B,C,H,W) logits, int64 labels; forward and gradient in one kernel.  Labels equal to
    ``ignore_index`` are left out of the mean (zero gradient); any other label outside [0, C) turns the loss into NaN
    (PyTorch raises there; see the kernel)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        logits = _dense(logits, "logits")
        labels = _req(labels, "labels", torch.int64).contiguous()
        B, Cc, H, W = logits.shape
        if tuple(labels.shape) != (B, H, W):
            raise WsdlError(f"cross entropy: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        need = logits.requires_grad
        dl = torch.empty_like(logits) if need else None
        inv = torch.empty(1, device=logits.device, dtype=torch.float32)
        ws = workspace(lib().wsdl_reduce_workspace(), logits.device)
        check(lib().wsdl_softmax_ce_fwd_bwd(_p(logits), _p(labels), _p(loss), _p(dl), _p(inv), B, Cc, H, W, 1.0,
                                            int(ignore_index), _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dl, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, inv = ctx.saved_tensors
        out = torch.empty_like(dl)
        sc = torch.empty_like(inv)
        check(lib().wsdl_mul(_p(_dense(g.reshape(1))), _p(inv), _p(sc), 1, _stream()))      # upstream gradient x 1 / #pixels
        check(lib().wsdl_scale_by_device_scalar(_p(dl), _p(sc), _p(out), dl.numel(), _stream()))
        return out, None, None


_CE_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


class _SoftmaxCEEx(torch.autograd.Function):
    """nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing) with an optional pixel weight: the same kernel
    with its options on (wsdl_softmax_ce_ex_fwd_bwd).  The gradient flows into the logits only."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, weight, pixel_weight, label_smoothing, reduction, keep_zeros=False):
        logits = _dense(logits, "logits")
        labels = _req(labels, "labels", torch.int64).contiguous()
        B, Cc, H, W = logits.shape
        if tuple(labels.shape) != (B, H, W):
            raise WsdlError(f"cross entropy: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        none = reduction == 2
        loss = torch.empty((B, H, W) if none else (), device=logits.device, dtype=torch.float32)
        need = logits.requires_grad
        dl = torch.empty_like(logits) if need else None
        inv = None if none else torch.empty(1, device=logits.device, dtype=torch.float32)
        ws = workspace(lib().wsdl_reduce_workspace(), logits.device)
        check(lib().wsdl_softmax_ce_ex_fwd_bwd(_p(logits), _p(labels), _p(loss), _p(dl), _p(inv), B, Cc, H, W, 1.0,
                                               int(ignore_index), _p(weight), _p(pixel_weight), float(label_smoothing),
                                               int(reduction), _p(ws), ws.numel(), _stream()))
        ctx.none = none
        ctx.keep_zeros = bool(keep_zeros)
        ctx.save_for_backward(dl, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, inv = ctx.saved_tensors
        if not ctx.none and not ctx.keep_zeros:
            return (_scaled_grad(dl, g, inv),) + (None,) * 7       # upstream gradient x 1 / denominator
        out = torch.empty_like(dl)
        if ctx.none:
            B, Cc, H, W = dl.shape
            check(lib().wsdl_scale_by_pixel(_p(dl), _p(_dense(g, "upstream gradient")), _p(out), B, Cc, H, W, _stream()))
        else:       # cross_entropy_mined: a pixel that is not selected has gradient 0 also when NOTHING is selected (sc = inf)
            sc = torch.empty_like(inv)
            check(lib().wsdl_mul(_p(_dense(g.reshape(1))), _p(inv), _p(sc), 1, _stream()))
            check(lib().wsdl_mining_scale_grad(_p(dl), _p(sc), _p(out), dl.numel(), _stream()))
        return out, None, None, None, None, None, None, None


def _scaled_grad(dl, g, inv=None):
    """The backward of a 0-dim loss whose kernel left its gradient ``dl`` on the device: ``dl`` x the upstream gradient ``g``
    (x ``inv``, the one-element factor a fused kernel left un-applied) - wsdl_mul where there is an ``inv``, then
    wsdl_scale_by_device_scalar; no host read."""
    out = torch.empty_like(dl)
    sc = _dense(g.reshape(1))
    if inv is not None:
        g, sc = sc, torch.empty_like(inv)
        check(lib().wsdl_mul(_p(g), _p(inv), _p(sc), 1, _stream()))
    check(lib().wsdl_scale_by_device_scalar(_p(dl), _p(sc), _p(out), dl.numel(), _stream()))
    return out


class _PairwiseAffinityLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, image, window, sigma_color, sigma_space, apply_softmax, normalise, cache=None):
        need = preds.requires_grad           # asked of the argument: the dense copy of a strided view, made here, never needs one
        preds, image = _dense(preds, "preds"), _dense(image, "image")
        B, Cc, H, W = preds.shape
        if tuple(image.shape) != (B, 3, H, W):
            raise WsdlError(f"pairwise loss: image {tuple(image.shape)} does not match preds {tuple(preds.shape)}")
        loss = torch.empty(B if normalise else 1, device=preds.device, dtype=torch.float32)
        dp = torch.empty_like(preds) if need else None
        ws = workspace(lib().wsdl_pairwise_workspace(B, H, W), preds.device)
        check(lib().wsdl_pairwise_affinity_loss_fwd_bwd(_p(preds), _p(image), _p(loss), _p(dp), B, Cc, H, W,
                                                        int(window), float(sigma_color), float(sigma_space or 0.0),
                                                        int(apply_softmax), int(normalise), _p(cache), _p(ws), ws.numel(),
                                                        _stream()))
        ctx.save_for_backward(dp)
        ctx.normalise = normalise
        return loss if normalise else loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        if ctx.normalise:
            # per-image upstream gradients: one scale launch per image (B is small on this path)
            out = torch.empty_like(dp)
            g = _dense(g.reshape(-1))
            n = dp[0].numel()
            for b in range(dp.shape[0]):
                check(lib().wsdl_scale_by_device_scalar(_p(dp[b]), _p(g[b:b + 1]), _p(out[b]), n, _stream()))
        else:
            out = torch.empty_like(dp)
            check(lib().wsdl_scale_by_device_scalar(_p(dp), _p(_dense(g.reshape(1))), _p(out), dp.numel(), _stream()))
        return out, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------ functional API
def conv_bn_act(x, weight, gamma, beta, running_mean, running_var, stride, pad, dil, relu, residual=None,
                momentum=0.1, eps=1e-5, training=True, cache=None, passthrough=False, link=None, out_holder=None):
    """passthrough=True returns (y, x'): x' is x routed through this node, to be used as the identity branch so that
    its gradient is summed in the dgrad epilogue (train mode; eval mode returns x itself)."""
    if training:
        bump_stats_epoch()          # running statistics are about to be rewritten behind torch's back
        return _ConvBNAct.apply(x, weight, gamma, beta, residual, running_mean, running_var, stride, pad, dil,
                                bool(relu), momentum, eps, cache, bool(passthrough), link, out_holder)
    key = _cache_key(gamma, beta, running_mean, running_var) if cache is not None else None
    if cache is not None and cache.get("fold_key") == key:
        scale, shift = cache["fold"]
    else:
        scale, shift = bn_fold(gamma.detach(), beta.detach(), running_mean, running_var, eps)
        if cache is not None:
            cache["fold_key"], cache["fold"] = key, (scale, shift)
    y = _ConvAffineAct.apply(x, weight, scale, shift, residual, stride, pad, dil, bool(relu), False, cache)
    return (y, x) if passthrough else y


def conv_bias_act(x, weight, bias=None, stride=1, pad=0, dil=1, relu=False, residual=None, cache=None):
    return _ConvAffineAct.apply(x, weight, None, bias, residual, stride, pad, dil, bool(relu), bias is not None, cache)


def linear(x, weight, bias=None):
    """nn.Linear on (B,F) as a 1x1 convolution over a 1x1 map."""
    B, Fin = x.shape
    y = conv_bias_act(x.reshape(B, Fin, 1, 1), weight.reshape(weight.shape[0], Fin, 1, 1), bias)
    return y.reshape(B, -1)


def max_pool_3x3_s2(x):
    return _MaxPool3x3s2.apply(x)


def global_avg_pool(x):
    return _GlobalAvgPool.apply(x)


def class_logit_head(h, weight, bias=None, class_idx=None):
    """LayerCAM's class-logit head on layer4's output h (B,C,H,W): logits = fc(avgpool(h)), the class per image (class_idx or the
    arg-max) and d logit[class] / d h = weight[class] / HW per pixel - wsdl_class_logit_head; fc's own parameter gradients are
    not formed.  Returns (logits (B,K), cls (B,) int32, dh like h)."""
    h = _dense(h, "h")
    B, Cc, H, W = h.shape
    K = weight.shape[0]
    if tuple(weight.shape) != (K, Cc) or not weight.is_contiguous() or weight.dtype != torch.float32:
        raise WsdlError("class_logit_head: weight must be a contiguous float32 (classes, channels) tensor")
    pooled = torch.empty(B, Cc, device=h.device, dtype=torch.float32)
    check(lib().wsdl_global_avgpool_fwd(_p(h), _p(pooled), B * Cc, H * W, _stream()))
    logits = torch.empty(B, K, device=h.device, dtype=torch.float32)
    cls = torch.empty(B, device=h.device, dtype=torch.int32)
    dh = torch.empty_like(h)
    if class_idx is not None:
        class_idx = class_idx.to(device=h.device, dtype=torch.int64).contiguous().view(-1)
        if class_idx.numel() != B:
            raise WsdlError("class_logit_head: one class index per image")
    check(lib().wsdl_class_logit_head(_p(pooled), _p(weight), _p(bias) if bias is not None else None,
                                      _p(class_idx) if class_idx is not None else None, _p(logits), _p(cls), _p(dh), B, Cc, K, H * W,
                                      _stream()))
    return logits, cls, dh


def bilinear_resize(x, size):
    return _Bilinear.apply(x, int(size[0]), int(size[1]))


def _out_planes(out):
    """(out, batch stride) of an output whose images are dense planes (a channel slice): written in place, never copied."""
    t, bs = _planes(out, "out")
    if t.data_ptr() != out.data_ptr():
        raise WsdlError("output tensor: images must be dense channel planes (a channel slice of an NCHW tensor)")
    return t, bs


def bilinear_into(x, out):
    """bilinear_resize of dense x written into ``out`` (B,C,H,W), which may be a channel slice of a wider tensor."""
    x = _dense(x, "x")
    B, Cc, h, w = x.shape
    out, y_bs = _out_planes(out)
    if out.shape[0] != B or out.shape[1] != Cc:
        raise WsdlError("bilinear_into: output does not match the input's batch / channels")
    check(lib().wsdl_bilinear_fwd(_p(x), _p(out), B, Cc, h, w, int(out.shape[2]), int(out.shape[3]), y_bs, _stream()))
    return out


def max_pool_2x2_ceil(x, out=None):
    """nn.MaxPool2d(2, 2, ceil_mode=True); x and ``out`` may be channel slices of wider tensors."""
    x, x_bs = _planes(x, "x")
    B, Cc, H, W = x.shape
    shape = (B, Cc, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != shape:
        raise WsdlError(f"max_pool_2x2_ceil: output {tuple(out.shape)} is not {shape}")
    out, y_bs = _out_planes(out)
    check(lib().wsdl_maxpool2x2_ceil_fwd(_p(x), _p(out), B, Cc, H, W, x_bs, y_bs, _stream()))
    return out


def side_output(x, weight, bias, s, residual=None, sigmoid=True, out=None, logits=None):
    """A 3x3 Cin -> 1 convolution with bias (+ residual (B,1,h,w)), then sigmoid(bilinear up-sample by s): BASNet's side outputs
    and RefUnet's tail (wsdl_side_output).  Returns (y (B,1,h*s,w*s), logits (B,1,h,w)); sigmoid=False: y holds the up-sampled
    logits."""
    x, x_bs = _planes(x, "x")
    B, Cin, h, w = x.shape
    if tuple(weight.shape) != (1, Cin, 3, 3) or bias is None or bias.numel() != 1:
        raise WsdlError(f"side_output: weight {tuple(weight.shape)} / bias is not a (1,{Cin},3,3) conv with a bias")
    if residual is not None:
        residual = _dense(residual, "residual")
        if tuple(residual.shape) != (B, 1, h, w):
            raise WsdlError("side_output: residual must be (B,1,h,w)")
    if logits is None:
        logits = torch.empty(B, 1, h, w, device=x.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(B, 1, h * s, w * s, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (B, 1, h * s, w * s):
        raise WsdlError("side_output: bad output shape")
    out, y_bs = _out_planes(out)
    check(lib().wsdl_side_output(_p(x), x_bs, _p(_dense(weight, "weight")), _p(_dense(bias, "bias")), _p(residual), B, Cin, h, w,
                                 int(s), _p(logits), _p(out), y_bs, int(bool(sigmoid)), _stream()))
    return out, logits


def saliency_u8(d):
    """(B,1,H,W) or (B,H,W) fp32 -> (B,H,W) uint8: norm_pred per image, then (p * 255).astype(uint8) (wsdl_saliency_u8)."""
    if d.dim() == 4:
        if d.shape[1] != 1:
            raise WsdlError("saliency_u8: one channel expected")
        d = d[:, 0]
    d = _dense(d, "d")
    B, H, W = d.shape
    out = torch.empty(B, H, W, device=d.device, dtype=torch.uint8)
    check(lib().wsdl_saliency_u8(_p(d), H * W, _p(out), B, H * W, _stream()))
    return out


def seg_counts(logits, labels, out=None, accumulate=False):
    """argmax over C of (B,C,H,W) fp32 logits vs (B,H,W) int64 labels -> int64 (3C+1,) on the device:
    [inter[C] | npred[C] | nlabel[C] | correct] (wsdl_seg_counts; 2 <= C <= 64).  ``out``: a dense int64 (3C+1,) row to
    write (``accumulate``: add to it instead of overwriting).  No host synchronisation."""
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise WsdlError("seg_counts: logits must be (B,C,H,W) float32")
    B, Cc, H, W = logits.shape
    if tuple(labels.shape) != (B, H, W) or labels.dtype != torch.int64:
        raise WsdlError(f"seg_counts: labels must be int64 {(B, H, W)}, got {labels.dtype} {tuple(labels.shape)}")
    logits = _dense(logits, "logits")
    _req(labels, "labels", torch.int64)
    labels = labels if labels.is_contiguous() else labels.contiguous()
    if out is None:
        out = torch.empty(3 * Cc + 1, device=logits.device, dtype=torch.int64)
        accumulate = False
    elif out.dtype != torch.int64 or out.numel() != 3 * Cc + 1 or not out.is_contiguous() or out.device != logits.device:
        raise WsdlError("seg_counts: out must be a dense int64 row of 3C+1 on the logits' device")
    check(lib().wsdl_seg_counts(_p(logits), _p(labels), _p(out), B, Cc, H * W, int(bool(accumulate)), _stream()))
    return out


# ---- Pillow's 8-bit resampling (csrc/pil_resize.hip) -------------------------------------------------------------------
PIL_BILINEAR, PIL_BICUBIC = 2, 3            # Pillow's Image.BILINEAR / Image.BICUBIC
PIL_MAX_SIDE = 16384
# one image of a batch: wsdl_pil_image_t
PIL_IMAGE_DTYPE = np.dtype([("src_off", np.int64), ("h", np.int32), ("w", np.int32), ("htab", np.int32), ("vtab", np.int32)])


def _pil_filter(filter):
    """'bilinear' / 'bicubic' or Pillow's enum value; any other value is refused by the library (wsdl_pil_coeffs)."""
    f = {"bilinear": PIL_BILINEAR, "bicubic": PIL_BICUBIC}.get(filter, filter)
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)):
        raise WsdlError(f"pil_resize: filter {filter!r}: 'bilinear' (2) or 'bicubic' (3)")
    return int(f)


def pil_coeffs(n_in, n_out, filter):
    """Pillow's resampling table of one axis (wsdl_pil_coeffs; host only): (ksize, bounds (n_out, 2) int32 = (xmin, xmax),
    coefficients (n_out, ksize) int32 with 22 fractional bits)."""
    f = _pil_filter(filter)
    ksize = C.c_int(0)
    check(lib().wsdl_pil_coeffs(int(n_in), int(n_out), f, C.byref(ksize), None, None))
    bounds = np.empty((int(n_out), 2), dtype=np.int32)
    kk = np.empty((int(n_out), ksize.value), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    check(lib().wsdl_pil_coeffs(int(n_in), int(n_out), f, C.byref(ksize), bounds.ctypes.data_as(ip), kk.ctypes.data_as(ip)))
    return ksize.value, bounds, kk


class PilTables:
    """The resampling tables of one device in one int32 arena, uploaded once per (in, out, filter) (Pet has a few hundred
    distinct side lengths, a table is ~10-50 KB).  ``offset`` returns a table's place in ``arena`` in int32 units.  When the
    arena grows the old contents are copied on the current stream, so offsets handed out earlier stay valid."""

    def __init__(self, device, capacity=1 << 20):
        self.device = torch.device(device)
        self.arena = torch.empty(capacity, dtype=torch.int32, device=self.device)
        self.used = 0
        self._offsets = {}
        self._lock = threading.Lock()

    def offset(self, n_in, n_out, filter):
        key = (int(n_in), int(n_out), int(filter))
        off = self._offsets.get(key)
        if off is not None:
            return off
        ksize, bounds, kk = pil_coeffs(*key)
        table = np.concatenate([np.array([ksize], dtype=np.int32), bounds.ravel(), kk.ravel()])
        with self._lock:
            off = self._offsets.get(key)
            if off is not None:
                return off
            if self.used + table.size > self.arena.numel():
                grown = torch.empty(max(2 * self.arena.numel(), self.used + table.size), dtype=torch.int32, device=self.device)
                grown[:self.used].copy_(self.arena[:self.used])
                self.arena = grown
            off = self.used
            self.arena[off:off + table.size].copy_(torch.from_numpy(table))
            self.used += table.size
            self._offsets[key] = off
        return off


_PIL_TABLES = {}


def pil_tables(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise WsdlError(f"pil_resize: the HIP path needs a device (got {device}); there is no CPU fallback")
    key = device.index if device.index is not None else _cur_device()
    if key not in _PIL_TABLES:
        _PIL_TABLES[key] = PilTables(torch.device("cuda", key))
    return _PIL_TABLES[key]


def pil_describe(shapes, offsets, size, filter, device):
    """The descriptor rows (PIL_IMAGE_DTYPE) of images of ``shapes`` [(h, w), ...] at byte ``offsets`` of the source buffer,
    for a resize to ``size`` = (out_h, out_w); their tables are made and uploaded on first use."""
    f = _pil_filter(filter)
    out_h, out_w = (int(v) for v in size)
    tables = pil_tables(device)
    desc = np.empty(len(shapes), dtype=PIL_IMAGE_DTYPE)
    for i, ((h, w), off) in enumerate(zip(shapes, offsets)):
        desc[i] = (off, h, w, tables.offset(w, out_w, f), tables.offset(h, out_h, f))
    return desc


def pil_resize(src, desc, channels, size, *, out=None, out_f32=None, lut=None):
    """Pillow's ``Image.resize(size, BILINEAR | BICUBIC)`` of N 8-bit images of different sizes in one launch
    (wsdl_pil_resize_u8), bit for bit.

    src       1-D uint8 device buffer: the images as ``np.asarray(pil_image)`` yields them (h x w x C interleaved), each at
              the byte offset its descriptor names;
    desc      the descriptors of ``pil_describe`` (which also fixes the filter): a numpy array (checked against ``src``
              and uploaded) or a device uint8 tensor that holds N of them (8-byte aligned);
    channels  1 or 3; size = (out_h, out_w).
    Returns the planar (N, C, out_h, out_w) uint8 (``out``, allocated when neither output is given) and / or writes
    ``out_f32`` = ``lut[c, u8]`` (float32, same shape; ``lut`` (C, 256) float32 on the device).  Returns ``(out, out_f32)``.
    Current stream, no host synchronisation on results, no CPU fallback."""
    _req(src, "pil_resize: src", torch.uint8)
    if src.dim() != 1 or not src.is_contiguous():
        raise WsdlError("pil_resize: src must be a dense 1-D uint8 buffer")
    Cc = int(channels)
    if Cc not in (1, 3):
        raise WsdlError(f"pil_resize: channels = {channels}, supported 1 and 3")
    out_h, out_w = (int(v) for v in size)
    if not (1 <= out_h <= PIL_MAX_SIDE and 1 <= out_w <= PIL_MAX_SIDE):
        raise WsdlError(f"pil_resize: size {tuple(size)}: side lengths 1..{PIL_MAX_SIDE}")
    itemsize = PIL_IMAGE_DTYPE.itemsize
    if isinstance(desc, np.ndarray):
        if desc.dtype != PIL_IMAGE_DTYPE or desc.ndim != 1 or len(desc) == 0:
            raise WsdlError("pil_resize: desc must be a non-empty 1-D array of PIL_IMAGE_DTYPE")
        end = desc["src_off"] + desc["h"].astype(np.int64) * desc["w"] * Cc
        if (desc["src_off"] < 0).any() or (desc["h"] < 1).any() or (desc["w"] < 1).any() or end.max() > src.numel():
            raise WsdlError("pil_resize: a descriptor points outside src")
        n = len(desc)
        desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(src.device)
    else:
        _req(desc, "pil_resize: desc", torch.uint8)
        if desc.dim() != 1 or not desc.is_contiguous() or desc.numel() == 0 or desc.numel() % itemsize or desc.data_ptr() % 8:
            raise WsdlError("pil_resize: a device desc must be dense uint8, 8-byte aligned, a multiple of %d bytes" % itemsize)
        n = desc.numel() // itemsize
    shape = (n, Cc, out_h, out_w)
    if out is None and out_f32 is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    for t, name, dt in ((out, "out", torch.uint8), (out_f32, "out_f32", torch.float32)):
        if t is not None:
            _req(t, "pil_resize: " + name, dt)
            if t.numel() != n * Cc * out_h * out_w or not t.is_contiguous() or t.device != src.device:
                raise WsdlError(f"pil_resize: {name} must be a dense {dt} tensor of {shape} on src's device")
    if out_f32 is not None:
        if lut is None:
            raise WsdlError("pil_resize: out_f32 needs lut, the (C, 256) float32 table")
        _req(lut, "pil_resize: lut")
        if tuple(lut.shape) != (Cc, 256) or not lut.is_contiguous() or lut.device != src.device:
            raise WsdlError(f"pil_resize: lut must be a dense float32 {(Cc, 256)} on src's device")
    tables = pil_tables(src.device)
    check(lib().wsdl_pil_resize_u8(_p(src), _p(desc), _p(tables.arena), n, Cc, out_h, out_w, _p(out), _p(out_f32),
                                   _p(lut) if out_f32 is not None else None, _stream()))
    return out, out_f32


def pil_pack(arrays, channels):
    """[H x W x C (or H x W for C = 1) uint8 arrays] -> (one flat uint8 array, shapes, byte offsets): the source layout of
    ``pil_resize``."""
    Cc = int(channels)
    shapes, offsets, total = [], [], 0
    flat = []
    for a in arrays:
        a = np.asarray(a)
        ok = a.dtype == np.uint8 and (a.ndim == 3 and a.shape[2] == Cc or a.ndim == 2 and Cc == 1)
        if not ok:
            raise WsdlError(f"pil_resize: an H x W x {Cc} uint8 array expected, got {a.dtype} {a.shape}")
        shapes.append((a.shape[0], a.shape[1]))
        offsets.append(total)
        flat.append(np.ascontiguousarray(a).reshape(-1))
        total += flat[-1].size
    return (np.concatenate(flat) if flat else np.empty(0, np.uint8)), shapes, offsets


def pil_resize_arrays(arrays, size, filter, channels=3, device="cuda", *, out=None, out_f32=None, lut=None):
    """``pil_resize`` of a list of host arrays: packed, copied and resized in one launch."""
    flat, shapes, offsets = pil_pack(arrays, channels)
    if not shapes:
        raise WsdlError("pil_resize: no images")
    desc = pil_describe(shapes, offsets, size, filter, device)
    return pil_resize(torch.from_numpy(flat).to(device), desc, channels, size, out=out, out_f32=out_f32, lut=lut)


# ---- joint image / label augmentation of a training batch (csrc/augment.hip) -------------------------------------------
AUGMENT_FILLS = {"ignore": 0, "reflect": 1}         # WSDL_AUGMENT_IGNORE / WSDL_AUGMENT_REFLECT
AUGMENT_MAX_SIDE = 16384


def augment_batch(images, labels, idx, params, out_size=None, *, lut=None, label_lut=None, fill="ignore", pad_value=0.0,
                  pad_label=-100):
    """Gather, warp and map a batch of a device-resident dataset in one launch (wsdl_augment_batch; the reference has no
    augmentation).

    images     (N,C,H,W) dense, C in {1, 3}: float32, or uint8 read through ``lut`` (C,256) float32 (``lut[c, u8]``);
    labels     (N,H,W) dense uint8; ``label_lut``: (256,) int64, raw byte -> class (None: the byte itself);
    idx        (B,) int64 on the device: item b reads source row ``idx[b]``;
    params     (B,8) float32 on the device: ``a00 a01 a02 a10 a11 a12 gain bias`` per item - the affine map from output to
               source pixel coordinates and the photometric map (``augment.Augment.draw``; include/wsdl_hip.h states the
               arithmetic);
    out_size   (out_h, out_w), default the source's;
    fill       "ignore": output pixels whose source point lies outside the image get ``pad_value`` / ``pad_label``;
               "reflect": the source is mirrored about its borders, nothing is padded.
    Returns ``(images_out (B,C,out_h,out_w) float32, labels_out (B,out_h,out_w) int64)``.  Current stream, no host
    synchronisation, no CPU fallback."""
    for t, name in ((images, "images"), (labels, "labels"), (idx, "idx"), (params, "params"), (lut, "lut"),
                    (label_lut, "label_lut")):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise WsdlError(f"augment_batch: {name}: the HIP path needs a device tensor "
                            f"(got {t.device if torch.is_tensor(t) else type(t).__name__}); there is no CPU fallback")
    if images.dim() != 4 or images.dtype not in (torch.float32, torch.uint8) or not images.is_contiguous():
        raise WsdlError("augment_batch: images must be a dense (N,C,H,W) float32 or uint8 tensor")
    N, Cc, H, W = images.shape
    if Cc not in (1, 3):
        raise WsdlError(f"augment_batch: C = {Cc}, supported 1 and 3")
    dev = images.device
    _req(labels, "augment_batch: labels", torch.uint8)
    if tuple(labels.shape) != (N, H, W) or not labels.is_contiguous() or labels.device != dev:
        raise WsdlError(f"augment_batch: labels must be a dense uint8 {(N, H, W)} on the images' device, got {tuple(labels.shape)}")
    _req(idx, "augment_batch: idx", torch.int64)
    _req(params, "augment_batch: params")
    B = idx.numel()
    if idx.dim() != 1 or B == 0 or not idx.is_contiguous() or idx.device != dev:
        raise WsdlError("augment_batch: idx must be a dense non-empty (B,) int64 tensor on the images' device")
    if tuple(params.shape) != (B, 8) or not params.is_contiguous() or params.device != dev:
        raise WsdlError(f"augment_batch: params must be a dense float32 {(B, 8)} on the images' device, got {tuple(params.shape)}")
    u8 = images.dtype == torch.uint8
    if u8:
        if lut is None:
            raise WsdlError("augment_batch: a uint8 source needs lut, the (C, 256) float32 table")
        _req(lut, "augment_batch: lut")
        if tuple(lut.shape) != (Cc, 256) or not lut.is_contiguous() or lut.device != dev:
            raise WsdlError(f"augment_batch: lut must be a dense float32 {(Cc, 256)} on the images' device")
    elif lut is not None:
        raise WsdlError("augment_batch: lut goes with a uint8 source")
    if label_lut is not None:
        _req(label_lut, "augment_batch: label_lut", torch.int64)
        if label_lut.numel() != 256 or not label_lut.is_contiguous() or label_lut.device != dev:
            raise WsdlError("augment_batch: label_lut must be a dense int64 table of 256 on the images' device")
    if fill not in AUGMENT_FILLS:
        raise WsdlError(f"augment_batch: fill {fill!r}: 'ignore' or 'reflect'")
    out_h, out_w = (H, W) if out_size is None else (int(v) for v in out_size)
    if not (1 <= out_h <= AUGMENT_MAX_SIDE and 1 <= out_w <= AUGMENT_MAX_SIDE):
        raise WsdlError(f"augment_batch: out_size {(out_h, out_w)}: side lengths 1..{AUGMENT_MAX_SIDE}")
    images_out = torch.empty(B, Cc, out_h, out_w, dtype=torch.float32, device=dev)
    labels_out = torch.empty(B, out_h, out_w, dtype=torch.int64, device=dev)
    check(lib().wsdl_augment_batch(_p(images), int(u8), _p(lut), _p(labels), _p(label_lut), _p(idx), _p(params), N, Cc, H, W,
                                   B, out_h, out_w, AUGMENT_FILLS[fill], float(pad_value), int(pad_label), _p(images_out),
                                   _p(labels_out), _stream()))
    return images_out, labels_out


DROPOUT_SEED_OFFSET = [0]      # dp.init_distributed: a different offset on every rank, so replicas draw different masks


def dropout(x, p, training=True, seed=None, mask=None, counter=None):
    """``counter``: a device int64 call counter (nn.Dropout keeps one): the mask then depends on (seed, counter) and the
    module draws its host seed only once - required for hipGraph replay, where a per-call host seed would be frozen."""
    if not training or p == 0.0:
        return x
    if seed is None:
        seed = (int(torch.randint(0, 2 ** 62, (1,)).item()) + DROPOUT_SEED_OFFSET[0]) % (1 << 62)
    return _Dropout.apply(x, p, seed, mask, counter)


def concat_channels(xs):
    return _ConcatChannels.apply(*xs)


def add_act(a, b, relu=False):
    return _AddAct.apply(a, b, bool(relu))


def check_cross_entropy_options(reduction, label_smoothing):
    """ValueError for a reduction or a smoothing factor the cross entropy does not know (no device needed)."""
    if reduction not in _CE_REDUCTIONS:
        raise ValueError(f"cross_entropy: reduction {reduction!r}: 'mean', 'sum' or 'none'")
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"cross_entropy: label_smoothing {label_smoothing!r} must be a number in [0, 1]")


def cross_entropy(logits, labels, ignore_index=-100, *, weight=None, label_smoothing=0.0, reduction="mean",
                  pixel_weight=None):
    """``F.cross_entropy`` on (B,C,H,W) logits and int64 (B,H,W) labels, forward and gradient in one kernel.

    ``weight`` (C,) float32 class weights, ``label_smoothing`` in [0, 1] and ``reduction`` 'mean' | 'sum' | 'none' are
    PyTorch's; ``pixel_weight`` (B,H,W) float32, finite and >= 0 (not checked on the device), multiplies the loss of each
    pixel - a pixel of weight 0 is an ignored pixel.  'mean' divides by the sum of ``pixel_weight * weight[label]`` over
    the pixels that are not ignored (PyTorch's denominator: the target classes only, also with smoothing); where that is
    0 the result is NaN.  A label outside [0, C) other than ``ignore_index`` gives NaN ('none': at that pixel only).
    Weights are constants: the gradient flows into ``logits`` only.  With every option at its default this is the plain
    kernel call (wsdl_softmax_ce_fwd_bwd)."""
    check_cross_entropy_options(reduction, label_smoothing)
    if weight is None and pixel_weight is None and label_smoothing == 0.0 and reduction == "mean":
        return _SoftmaxCE.apply(logits, labels, ignore_index)
    return _cross_entropy_ex(logits, labels, ignore_index, weight, label_smoothing, reduction, pixel_weight)


def _cross_entropy_ex(logits, labels, ignore_index, weight, label_smoothing, reduction, pixel_weight, keep_zeros=False):
    """``cross_entropy`` with options, after their check.  ``keep_zeros``: see ``_SoftmaxCEEx.backward``."""
    if logits.dim() != 4:
        raise WsdlError(f"cross entropy: logits {tuple(logits.shape)} must be (B,C,H,W)")
    B, Cc, H, W = logits.shape
    for t, name, shape in ((weight, "weight", (Cc,)), (pixel_weight, "pixel_weight", (B, H, W))):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise WsdlError(f"cross entropy: {name} must be a float32 tensor")
        if tuple(t.shape) != shape:
            raise WsdlError(f"cross entropy: {name} {tuple(t.shape)} must be {shape}")
        if t.device != logits.device:
            raise WsdlError(f"cross entropy: {name} is on {t.device}, the logits on {logits.device}")
    weight = None if weight is None else weight.detach().contiguous()
    pixel_weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    return _SoftmaxCEEx.apply(logits, labels, ignore_index, weight, pixel_weight, float(label_smoothing),
                              _CE_REDUCTIONS[reduction], keep_zeros)


def class_weights_from_labels(labels, C, ignore=None, mode="inverse"):
    """float32 (C,) class weights on the device from the pixel counts n_c of int64 ``labels`` (``ignore`` left out):
    ``mode='inverse'`` N / (C n_c) with N = sum_c n_c, ``'median'`` median(n) / n_c (the median of all C counts,
    the ignored class counting as 0); a class without a pixel gets weight 0.  The counts are ``iou_counts(labels, labels, C, ignore)[..., 0]``;
    no host synchronisation."""
    if mode not in ("inverse", "median"):
        raise ValueError(f"class_weights_from_labels: mode {mode!r}: 'inverse' or 'median'")
    n = iou_counts(labels, labels, C, ignore)[0, :, 0].to(torch.float64)
    if ignore is not None and 0 <= int(ignore) < int(C):
        n = n * torch.tensor([float(c != int(ignore)) for c in range(int(C))], dtype=torch.float64).to(n.device, non_blocking=True)
    num = n.sum() / float(C) if mode == "inverse" else torch.quantile(n, 0.5)      # the mean of the two middle counts for an even C
    return torch.where(n > 0, num / n.clamp_min(1.0), torch.zeros_like(n)).to(torch.float32)


def _out_tensor(out, key, shape, dtype, device):
    """``out[key]`` when it is a dense device tensor of that shape and type (the caller's buffer: its address stays), else a new
    one, stored under ``key`` when ``out`` is a dict."""
    t = None if out is None else out.get(key)
    if not (torch.is_tensor(t) and tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.device == device
            and t.is_contiguous()):
        t = torch.empty(shape, device=device, dtype=dtype)
        if out is not None:
            out[key] = t
    return t


def kth_value(x, k=0, frac=0.0, *, largest=True, valid=None, segments=1, out=None):
    """The ``K``-th largest (``largest=False``: smallest) value of each of the ``segments`` equal runs of the dense float32
    device tensor ``x``, with ``K = min(n, k + floor(frac * n))`` computed ON THE DEVICE from ``n``, the number of candidates
    of the run: its elements that are not NaN and, with ``valid`` (uint8 / bool, the shape of ``x``), are marked there.
    Returns ``(value, n_valid)``: float32 and int64 device tensors of ``segments`` entries; no host synchronisation.

    ``value`` is an element of ``x`` bit for bit (of -0.0 and +0.0 either may come back); ``K == 0`` (an empty run included)
    gives +inf for ``largest`` and -inf otherwise, so that ``x >= value`` / ``x <= value`` keeps nothing.  A radix select in
    four launches (wsdl_kth_value); bitwise reproducible.  ``out``: a dict whose ``"value"`` / ``"n_valid"`` tensors receive
    the results."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"kth_value: k {k!r} must be an int >= 0")
    if isinstance(frac, bool) or not isinstance(frac, (int, float)) or not 0.0 <= frac <= 1.0:
        raise ValueError(f"kth_value: frac {frac!r} must be a number in [0, 1]")
    if isinstance(segments, bool) or not isinstance(segments, int) or segments < 1:
        raise ValueError(f"kth_value: segments {segments!r} must be an int >= 1")
    x = _req(x, "kth_value: x").detach()
    x = x if x.is_contiguous() else x.contiguous()
    if x.numel() == 0 or x.numel() % segments:
        raise WsdlError(f"kth_value: {x.numel()} elements do not split into {segments} non-empty segments")
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.uint8, torch.bool) or valid.shape != x.shape or valid.device != x.device:
            raise WsdlError("kth_value: valid must be a uint8 / bool device tensor of the shape of x")
        valid = valid if valid.is_contiguous() else valid.contiguous()
    value = _out_tensor(out, "value", (segments,), torch.float32, x.device)
    n_valid = _out_tensor(out, "n_valid", (segments,), torch.int64, x.device)
    ws = workspace(lib().wsdl_kth_workspace(segments), x.device)
    check(lib().wsdl_kth_value(_p(x), _p(valid), x.numel() // segments, segments, int(bool(largest)), int(k), float(frac),
                               _p(value), _p(n_valid), _p(ws), ws.numel(), _stream()))
    return value, n_valid


_MINING_MODES = {"hard": 0, "trim": 1}


def check_mining_options(mode, thresh, min_kept, drop_frac, scope, reduction, label_smoothing=0.0):
    """ValueError for an option ``cross_entropy_mined`` does not know (no device needed)."""
    if mode not in _MINING_MODES:
        raise ValueError(f"cross_entropy_mined: mode {mode!r}: 'hard' or 'trim'")
    if scope not in ("batch", "image"):
        raise ValueError(f"cross_entropy_mined: scope {scope!r}: 'batch' or 'image'")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"cross_entropy_mined: reduction {reduction!r}: 'mean' or 'sum'")
    check_cross_entropy_options(reduction, label_smoothing)
    if thresh is not None and (isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not 0.0 < thresh <= 1.0):
        raise ValueError(f"cross_entropy_mined: thresh {thresh!r} must be None or a number in (0, 1]")
    if isinstance(min_kept, bool) or not isinstance(min_kept, int) or min_kept < 0:
        raise ValueError(f"cross_entropy_mined: min_kept {min_kept!r} must be an int >= 0")
    if isinstance(drop_frac, bool) or not isinstance(drop_frac, (int, float)) or not 0.0 <= drop_frac < 1.0:
        raise ValueError(f"cross_entropy_mined: drop_frac {drop_frac!r} must be a number in [0, 1)")


def cross_entropy_mined(logits, labels, ignore_index=-100, *, mode, thresh=None, min_kept=0, drop_frac=0.0, scope="batch",
                        weight=None, label_smoothing=0.0, pixel_weight=None, reduction="mean", stats=None):
    """``ops.cross_entropy`` over the pixels their own loss selects - hard-pixel mining or loss trimming - with the selection
    made on the device: no ``topk`` / ``sort``, no host read of a pixel count, so a launch plan holds the step.

    The ranking statistic is ``nll = -log softmax(logits)[label]`` (no class weights, no smoothing), over the valid pixels:
    label != ``ignore_index`` and ``pixel_weight`` != 0.  ``scope="batch"`` ranks the whole batch, ``"image"`` each image
    by itself.  With ``n`` valid pixels in the scope:

    ``mode="hard"`` (OHEM, bootstrapped cross entropy): keep the pixels whose true-class probability is at most ``thresh``,
    and at least ``min_kept`` per image of them (``scope="batch"``: ``min_kept * B`` in the batch) - that is
    ``nll >= min(tau, -log(thresh))`` with ``tau`` the ``min(n, K)``-th largest ``nll``; ``thresh=None`` keeps exactly the
    ``K`` hardest (``K == 0``: none).  ``mode="trim"`` (small-loss selection against label noise): drop the
    ``floor(drop_frac * n)`` pixels of largest loss - keep ``nll <= tau``, ``tau`` the ``(floor(drop_frac * n) + 1)``-th
    largest; ``drop_frac=0`` keeps everything.  The rule is INCLUSIVE: pixels that tie with ``tau`` are all kept, so hard
    mode keeps at least ``K`` and trim mode drops at most ``floor(drop_frac * n)``; mmsegmentation's OHEM sampler is strict
    at the boundary (``prob < threshold``) and differs from this exactly on the ties.

    The result is ``ops.cross_entropy(logits, labels, ignore_index, weight=, label_smoothing=, reduction=,
    pixel_weight=m)`` with ``m`` = ``pixel_weight`` (or 1) on the kept pixels and 0 elsewhere: the gradient flows through
    that call only, the selection is a constant.  'mean' divides by the sum of ``m * weight[label]``; nothing kept gives NaN
    ('sum': 0) with a gradient of zeros, as torch's cross entropy over ignored pixels only (a pixel that is not selected
    has gradient 0 whatever the denominator is; the kept pixels' gradients are those of that call bit for bit).  A label outside [0, C) other than ``ignore_index`` keeps its weight and makes the loss NaN, as without mining.

    ``stats``: a caller-owned dict; its device tensors ``"threshold"`` (float32: ``tau`` as selected, before the ``thresh``
    cap of hard mode), ``"kept"`` and ``"valid"`` (int64), one entry per scope segment, and ``"selection"`` (float32
    (B,H,W): ``m``) are filled in place where they have the right shape and created otherwise.  Nothing is read on the host."""
    check_mining_options(mode, thresh, min_kept, drop_frac, scope, reduction, label_smoothing)
    if logits.dim() != 4:
        raise WsdlError(f"cross entropy: logits {tuple(logits.shape)} must be (B,C,H,W)")
    B, Cc, H, W = logits.shape
    dev = logits.device
    labels = _req(labels, "labels", torch.int64).contiguous()
    if pixel_weight is not None:
        if not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.float32 or tuple(pixel_weight.shape) != (B, H, W) \
                or pixel_weight.device != dev:
            raise WsdlError(f"cross entropy: pixel_weight must be a float32 {(B, H, W)} tensor on {dev}")
        pixel_weight = pixel_weight.detach().contiguous()
    segments = B if scope == "image" else 1
    n = B * H * W
    nll = cross_entropy(logits.detach(), labels, ignore_index, reduction="none")
    valid = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    check(lib().wsdl_mining_valid(_p(labels), int(ignore_index), _p(pixel_weight), _p(valid), n, _stream()))
    if mode == "hard":
        k, frac = int(min_kept) * (B if scope == "batch" else 1), 0.0
        cap = float("inf") if thresh is None else float(np.float32(-np.log(np.float64(thresh))))
    else:
        k, frac, cap = 1, float(drop_frac), float("inf")
    tau = _out_tensor(stats, "threshold", (segments,), torch.float32, dev)
    n_valid = _out_tensor(stats, "valid", (segments,), torch.int64, dev)
    kth_value(nll, k, frac, largest=True, valid=valid, segments=segments, out={"value": tau, "n_valid": n_valid})
    m = _out_tensor(stats, "selection", (B, H, W), torch.float32, dev)
    kept = _out_tensor(stats, "kept", (segments,), torch.int64, dev)
    ws = workspace(lib().wsdl_mining_weights_workspace(segments), dev)
    check(lib().wsdl_mining_weights(_p(nll), _p(valid), _p(pixel_weight), _p(tau), cap, _MINING_MODES[mode], n // segments,
                                    segments, _p(m), _p(kept), _p(ws), ws.numel(), _stream()))
    return _cross_entropy_ex(logits, labels, ignore_index, weight, label_smoothing, reduction, m, keep_zeros=True)


_NO_LABEL = -(1 << 62)         # "ignore=None": a value no label has


def _ignore(ignore):
    return _NO_LABEL if ignore is None else int(ignore)


class _LovaszSoftmax(torch.autograd.Function):
    """lovasz_softmax(probas, labels, classes, per_image, ignore) - reference
    TraditionalModel/LossFunctions/Lovasz-Softmax_Loss.py:146-211; loss and d loss / d probas in one call.  Every (image
    or batch) x class is a segment of a device-wide sort (csrc/lovasz_seg.hip): a class list (``classes``) is ONE sort of
    all its entries; 'present' / 'all' (``classes`` a bool: all) sort class after class."""

    @staticmethod
    def forward(ctx, probas, labels, classes, per_image, ignore):
        probas = _dense(probas, "probas")
        labels = _req(labels, "labels", torch.int64).contiguous()
        B, Cc, H, W = probas.shape
        if tuple(labels.shape) != (B, H, W):
            raise WsdlError(f"lovasz_softmax: labels {tuple(labels.shape)} do not match probas {tuple(probas.shape)}")
        loss = torch.empty((), device=probas.device, dtype=torch.float32)
        dp = torch.empty_like(probas) if ctx.needs_input_grad[0] else None       # (a copy made dense above requires no grad)
        if isinstance(classes, bool):
            ws = workspace(_ws_bytes("wsdl_lovasz_softmax_workspace", B, Cc, H, W, int(per_image)), probas.device)
            check(lib().wsdl_lovasz_softmax_fwd_bwd(_p(probas), _p(labels), _p(loss), _p(dp), B, Cc, H, W, int(classes),
                                                    int(per_image), int(ignore), _p(ws), ws.numel(), _stream()))
        else:
            cls = (C.c_int * len(classes))(*classes)
            ws = workspace(_ws_bytes("wsdl_lovasz_softmax_classes_workspace", B, Cc, H, W, len(classes), int(per_image)),
                           probas.device)
            check(lib().wsdl_lovasz_softmax_classes_fwd_bwd(_p(probas), _p(labels), _p(loss), _p(dp), B, Cc, H, W,
                                                            C.cast(cls, C.c_void_p), len(classes), int(per_image), int(ignore),
                                                            _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None, None, None, None


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None):
    """probas (B,C,H,W) class probabilities (or (B,H,W): one sigmoid map), labels (B,H,W).  ``classes``: 'present', 'all'
    or a list of classes to average: every listed class is a term whether or not it occurs; with one sigmoid map (C = 1)
    the list has exactly one entry c and channel 0 is compared with ``labels == c`` (a longer list: ValueError, as in the
    reference).  Per image, an image whose pixels are all void is a zero term that counts in the mean (the reference
    returns an empty tensor there)."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)
    if not isinstance(classes, str):
        classes = [int(c) for c in classes]
        if not classes:
            raise WsdlError("lovasz_softmax: an empty class list")
        if probas.shape[1] == 1 and len(classes) > 1:
            raise ValueError("Sigmoid output possible only with 1 class")
    elif classes in ("present", "all"):
        classes = classes == "all"
    else:
        raise WsdlError("lovasz_softmax: classes must be 'present', 'all' or a list of classes")
    return _LovaszSoftmax.apply(probas, labels, classes, bool(per_image), _ignore(ignore))


class _LovaszHinge(torch.autograd.Function):
    """lovasz_hinge(logits, labels, per_image, ignore) - reference Lovasz-Softmax_Loss.py:71-119; loss and d loss / d logits
    in one call: one device-wide sort with the images as segments, one scan, one pass (csrc/lovasz_seg.hip)."""

    @staticmethod
    def forward(ctx, logits, labels, per_image, ignore):
        logits = _dense(logits, "logits")
        labels = _req(labels, "labels", torch.int64).contiguous()
        if logits.dim() == 4 and logits.shape[1] == 2:
            (B, _two, H, W), ch = logits.shape, 2
        elif logits.dim() == 3:
            (B, H, W), ch = logits.shape, 1
        else:
            raise WsdlError(f"lovasz_hinge: logits must be (B,H,W) or (B,2,H,W), got {tuple(logits.shape)}")
        if tuple(labels.shape) != (B, H, W):
            raise WsdlError(f"lovasz_hinge: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        ws = workspace(_ws_bytes("wsdl_lovasz_hinge_workspace", B, H, W, int(per_image)), logits.device)
        check(lib().wsdl_lovasz_hinge_fwd_bwd(_p(logits), _p(labels), _p(loss), _p(dl), B, ch, H, W, int(per_image),
                                              int(ignore), _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None


def lovasz_hinge(logits, labels, per_image=True, ignore=None):
    """Binary Lovasz hinge: logits (B,H,W), or (B,2,H,W) whose binary logit is plane 1 - plane 0; labels (B,H,W) int64 in
    {0, 1, ignore}.  Mean over the images (``per_image``) or one term for the batch; an image without a valid pixel is a
    zero term with zero gradient that still counts in the mean."""
    return _LovaszHinge.apply(logits, labels, bool(per_image), _ignore(ignore))


def iou_counts(preds, labels, C, ignore=None, per_image=False):
    """int64 (images, C, 2) on the device - images = B with ``per_image``, else 1: [..., 0] = #(label = c and pred = c),
    [..., 1] = #(label = c or (pred = c and label != ignore)) (wsdl_iou_counts).  preds, labels int64 (B,H,W).  No host
    synchronisation; ``iou_from_counts`` turns a host copy into the reference's numbers."""
    _req(preds, "preds", torch.int64)
    _req(labels, "labels", torch.int64)
    if preds.dim() < 2 or preds.shape != labels.shape:
        raise WsdlError(f"iou_counts: preds {tuple(preds.shape)} / labels {tuple(labels.shape)} must be equal (B,...) shapes")
    preds, labels = preds.contiguous(), labels.contiguous()
    B = preds.shape[0]
    HW = preds.numel() // max(B, 1)
    out = torch.empty((B if per_image else 1, int(C), 2), device=preds.device, dtype=torch.int64)
    check(lib().wsdl_iou_counts(_p(preds), _p(labels), _p(out), B, HW, int(C), int(bool(per_image)), _ignore(ignore), _stream()))
    return out


def iou_from_counts(counts, EMPTY=1.0, ignore=None):
    """Host arithmetic of the reference's ``iou`` (Lovasz-Softmax_Loss.py:46-65) on (images, C, 2) counts (anything
    ``np.asarray`` takes): per class - the ``ignore`` class left out - the mean over the images of intersection / union as
    Python floats, ``EMPTY`` where the union is 0; returns 100 x that as a float64 array."""
    counts = np.asarray(counts)
    ious = []
    for c in range(counts.shape[1]):
        if ignore is not None and c == ignore:
            continue
        per = [float(i) / float(u) if u else EMPTY for i, u in counts[:, c].tolist()]
        acc = per[0]
        for v in per[1:]:
            acc += v
        ious.append(acc if len(per) == 1 else acc / len(per))
    return 100 * np.array(ious)


def dice_from_counts(counts, EMPTY=1.0, ignore=None):
    """The hard Dice score from the (images, C, 2) counts of ``iou_counts`` (intersection i, union u), by the averaging rule
    of ``iou_from_counts``: per class - the ``ignore`` class left out - the mean over the images of ``2 i / (i + u)`` (i + u
    is |prediction| + |label|) as Python floats, ``EMPTY`` where the union is 0; returns 100 x that as a float64 array.
    Host arithmetic only."""
    counts = np.asarray(counts)
    dices = []
    for c in range(counts.shape[1]):
        if ignore is not None and c == ignore:
            continue
        per = [2.0 * float(i) / float(i + u) if u else EMPTY for i, u in counts[:, c].tolist()]
        acc = per[0]
        for v in per[1:]:
            acc += v
        dices.append(acc if len(per) == 1 else acc / len(per))
    return 100 * np.array(dices)


class _BinaryXLoss(torch.autograd.Function):
    """binary_xloss / StableBCELoss (reference Lovasz-Softmax_Loss.py:122-140) with a void label; forward and gradient in
    one kernel.  ``labels``: int64 labels, or float32 targets (no void label then)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore):
        logits = _dense(logits, "logits")
        soft = labels.dtype == torch.float32
        labels = _req(labels, "labels", torch.float32 if soft else torch.int64).contiguous()
        if labels.numel() != logits.numel():
            raise WsdlError(f"binary_xloss: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        inv = torch.empty(1, device=logits.device, dtype=torch.float32)
        ws = workspace(lib().wsdl_reduce_workspace(), logits.device)
        check(lib().wsdl_binary_xloss_fwd_bwd(_p(logits), None if soft else _p(labels), _p(labels) if soft else None, _p(loss),
                                              _p(dl), _p(inv), logits.numel(), int(ignore), _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dl, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, inv = ctx.saved_tensors
        out = torch.empty_like(dl)
        sc = torch.empty_like(inv)
        check(lib().wsdl_mul(_p(_dense(g.reshape(1))), _p(inv), _p(sc), 1, _stream()))      # upstream gradient x 1 / #valid pixels
        check(lib().wsdl_scale_by_device_scalar(_p(dl), _p(sc), _p(out), dl.numel(), _stream()))
        return out, None, None


def binary_xloss(logits, labels, ignore=None):
    """Mean over the pixels with ``labels != ignore`` of max(x,0) - x t + log(1 + exp(-|x|)); NaN when every pixel is void
    (the reference's mean of nothing), with a zero gradient.  ``labels`` int64, or float32 targets (every element counts)."""
    return _BinaryXLoss.apply(logits, labels, _ignore(ignore))


def _crf_rgb(images):
    """(B,H,W,3) uint8 as it is, or (B,3,H,W) float in [0,1] quantised on the device (truncation of x*255)."""
    if not images.is_cuda:
        raise WsdlError(f"dense_crf: the HIP path needs a device tensor (got {images.device}); there is no CPU fallback")
    if images.dtype == torch.uint8:
        if images.dim() != 4 or images.shape[-1] != 3:
            raise WsdlError(f"dense_crf: uint8 images must be (B,H,W,3), got {tuple(images.shape)}")
        return images.contiguous()
    if images.dim() != 4 or images.shape[1] != 3:
        raise WsdlError(f"dense_crf: float images must be (B,3,H,W), got {tuple(images.shape)}")
    images = _dense(images, "images")
    B, _, H, W = images.shape
    out = torch.empty(B, H, W, 3, device=images.device, dtype=torch.uint8)
    check(lib().wsdl_dense_crf_quantize(_p(images), _p(out), B, H, W, _stream()))
    return out


def _crf_ws(B, H, W, n_labels, device):
    n = lib().wsdl_dense_crf_workspace(B, H, W, int(n_labels))
    if n == 0:
        raise WsdlError(f"dense_crf: unsupported geometry B={B} H={H} W={W} n_labels={n_labels} (n_labels must be 2)")
    return workspace(n, device)


def dense_crf(images, cam=None, cam_thresh=None, n_iter=5, gauss=(1, 2), bilateral=(50, 5, 10), return_q=False,
              unary=None, n_labels=2):
    """Dense-CRF refinement (reference AlternatingDirectionCutLoss.py:183-204, pydensecrf defaults): masks (B,H,W) uint8
    [, Q (B,2,H,W) fp32].  images: (B,H,W,3) uint8 or (B,3,H,W) float in [0,1]; cam (B,H,W) fp32, values below
    ``cam_thresh`` set to 0; or ``unary`` (B,2,H,W) fp32 instead of the cam.  gauss = (sxy, compat),
    bilateral = (sxy, srgb, compat)."""
    rgb = _crf_rgb(images)
    B, H, W, _ = rgb.shape
    if (cam is None) == (unary is None):
        raise WsdlError("dense_crf: pass exactly one of cam and unary")
    if cam is not None:
        cam = _dense(cam, "cam")
        if tuple(cam.shape) != (B, H, W):
            raise WsdlError(f"dense_crf: cam {tuple(cam.shape)} does not match images (B,H,W) = {(B, H, W)}")
    else:
        unary = _dense(unary, "unary")
        if tuple(unary.shape) != (B, int(n_labels), H, W):
            raise WsdlError(f"dense_crf: unary {tuple(unary.shape)} is not (B,{n_labels},H,W) = {(B, n_labels, H, W)}")
    ws = _crf_ws(B, H, W, n_labels, rgb.device)
    mask = torch.empty(B, H, W, device=rgb.device, dtype=torch.uint8)
    q = torch.empty(B, 2, H, W, device=rgb.device, dtype=torch.float32) if return_q else None
    thr = float("-inf") if cam_thresh is None else float(cam_thresh)
    check(lib().wsdl_dense_crf(_p(rgb), _p(cam), _p(unary), thr, B, H, W, int(n_labels), int(n_iter), float(gauss[0]),
                               float(gauss[1]), float(bilateral[0]), float(bilateral[1]), float(bilateral[2]), _p(mask),
                               _p(q), _p(ws), ws.numel(), _stream()))
    return (mask, q) if return_q else mask


def dense_crf_lattice(images, bilateral, sxy, srgb=1.0):
    """Diagnostic: per-pixel lattice keys (B*H*W, d+1, d) int32, barycentric weights (B*H*W, d+1) and the number of
    lattice points per image (B) of one feature set (bilateral=False: (x, y)/sxy; True: also rgb/srgb)."""
    rgb = _crf_rgb(images)
    B, H, W, _ = rgb.shape
    d = 5 if bilateral else 2
    keys = torch.empty(B * H * W, d + 1, d, device=rgb.device, dtype=torch.int32)
    bary = torch.empty(B * H * W, d + 1, device=rgb.device, dtype=torch.float32)
    points = torch.empty(B, device=rgb.device, dtype=torch.int32)
    ws = _crf_ws(B, H, W, 2, rgb.device)
    check(lib().wsdl_dense_crf_lattice(_p(rgb), B, H, W, int(bool(bilateral)), float(sxy), float(srgb), _p(keys), _p(bary),
                                       _p(points), _p(ws), ws.numel(), _stream()))
    return keys, bary, points


def dense_crf_filter(images, values, bilateral, sxy, srgb=1.0, n_labels=2):
    """Diagnostic: one normalised filter application K~ values, values (B,2,H,W) fp32."""
    rgb = _crf_rgb(images)
    B, H, W, _ = rgb.shape
    values = _dense(values, "values")
    if tuple(values.shape) != (B, int(n_labels), H, W):
        raise WsdlError(f"dense_crf_filter: values {tuple(values.shape)} is not (B,{n_labels},H,W)")
    out = torch.empty_like(values)
    ws = _crf_ws(B, H, W, 2, rgb.device)
    check(lib().wsdl_dense_crf_filter(_p(rgb), _p(values), _p(out), B, H, W, int(n_labels), int(bool(bilateral)), float(sxy),
                                      float(srgb), _p(ws), ws.numel(), _stream()))
    return out


PAMR_DILATIONS = (1, 2, 4, 8, 12, 24)


def _pamr_dilations(dilations):
    """The dilations as a ctypes int array; ValueError for what is not 1 to 8 ints in [1, 64]."""
    try:
        dil = tuple(dilations)
    except TypeError:
        raise ValueError(f"pamr: dilations {dilations!r} must be a sequence of ints") from None
    if not 1 <= len(dil) <= 8 or any(isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= 64 for d in dil):
        raise ValueError(f"pamr: dilations {dil!r} must be 1 to 8 ints in [1, 64]")
    return dil, (C.c_int * len(dil))(*dil)


def pamr_workspace(B, K, C_, H, W, dilations=PAMR_DILATIONS):
    """Bytes of scratch ``pamr`` needs for images (B,K,H,W) and scores (B,C,H,W); 0 for a geometry outside the limits of
    include/wsdl_hip.h "PAMR" (K in [1,4], C in [1,32], 1 to 8 dilations in [1,64], non-empty planes).  Host-side: no device."""
    try:
        dil, _ = _pamr_dilations(dilations)
    except ValueError:
        return 0
    if not 1 <= int(K) <= 4:
        return 0
    return int(lib().wsdl_pamr_workspace(int(B), int(C_), int(H), int(W), len(dil)))


def _pamr_images(images):
    if not torch.is_tensor(images) or images.dim() != 4:
        raise WsdlError("pamr: images must be a (B,K,H,W) tensor")
    images = _dense(images.detach(), "pamr: images")
    if not 1 <= images.shape[1] <= 4 or images.numel() == 0:
        raise WsdlError(f"pamr: images {tuple(images.shape)} must be (B,K,H,W) with 1 <= K <= 4 and no empty dimension")
    return images


def pamr_affinity(images, dilations=PAMR_DILATIONS):
    """The propagation weights of ``pamr`` for float32 device images (B,K,H,W), 1 <= K <= 4: (B, 8 D, H, W) float32, plane
    8 i + j = neighbour j (raster order of the 3 x 3 ring without its centre) of dilation ``dilations[i]``, borders
    replicated; every pixel's weights are a softmax over its 8 D neighbours (include/wsdl_hip.h "PAMR").  They depend on
    the image only: a caller that refines several score maps against one batch computes them once (``pamr(affinity=)``)."""
    dil, arr = _pamr_dilations(dilations)
    images = _pamr_images(images)
    B, K, H, W = images.shape
    w = torch.empty(B, 8 * len(dil), H, W, device=images.device, dtype=torch.float32)
    check(lib().wsdl_pamr_affinity(_p(images), B, K, H, W, arr, len(dil), _p(w), _stream()))
    return w


def pamr(images, scores, num_iter=10, dilations=PAMR_DILATIONS, *, affinity=None, out=None):
    """Pixel-adaptive mask refinement (Araslanov & Roth, CVPR 2020): ``num_iter`` times ``m'_c(p) = sum_j w(p,j) m_c(q_j)``
    over the 8 D dilated neighbours of every pixel, ``w = pamr_affinity(images, dilations)``.  images (B,K,H,W), scores
    (B,C,H,W) with 1 <= C <= 32 on the same H x W, both float32 on the device -> refined scores (B,C,H,W).  Any score map:
    softmax probabilities, a raw CAM (C = 1), more than two classes.  Every output is a convex combination of inputs, so
    it stays inside their range; a constant map is a fixed point; ``num_iter=0`` copies.

    Not differentiable: the inputs are detached and the result has no ``grad_fn``.  One launch for the weights and one per
    iteration (per four score channels), no host read, bitwise reproducible - a launch plan can hold the call.
    ``affinity``: the weights when the caller already has them; ``out``: a dense float32 (B,C,H,W) device tensor that
    receives the result (it must not overlap ``scores``)."""
    if isinstance(num_iter, bool) or not isinstance(num_iter, int) or num_iter < 0:
        raise ValueError(f"pamr: num_iter {num_iter!r} must be an int >= 0")
    dil, arr = _pamr_dilations(dilations)
    images = _pamr_images(images)
    if not torch.is_tensor(scores) or scores.dim() != 4:
        raise WsdlError("pamr: scores must be a (B,C,H,W) tensor")
    scores = _dense(scores.detach(), "pamr: scores")
    B, K, H, W = images.shape
    Cc = scores.shape[1]
    if scores.device != images.device or scores.shape[0] != B or tuple(scores.shape[2:]) != (H, W):
        raise WsdlError(f"pamr: scores {tuple(scores.shape)} on {scores.device} do not match images {tuple(images.shape)} on "
                        f"{images.device}: same device, batch, height and width")
    nbytes = lib().wsdl_pamr_workspace(B, Cc, H, W, len(dil))
    if nbytes == 0:
        raise WsdlError(f"pamr: bad geometry, scores {tuple(scores.shape)} (1 <= C <= 32)")
    if affinity is None:
        affinity = pamr_affinity(images, dil)
    else:
        _req(affinity, "pamr: affinity")
        if tuple(affinity.shape) != (B, 8 * len(dil), H, W) or affinity.device != images.device or not affinity.is_contiguous():
            raise WsdlError(f"pamr: affinity must be a dense {(B, 8 * len(dil), H, W)} tensor on {images.device}")
        affinity = affinity.detach()
    if out is None:
        out = torch.empty_like(scores)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == scores.shape
              and out.device == scores.device and out.is_contiguous() and not out.requires_grad):
        raise WsdlError(f"pamr: out must be a dense float32 {tuple(scores.shape)} tensor on {scores.device} that needs no gradient")
    ws = workspace(nbytes, images.device)
    check(lib().wsdl_pamr_propagate(_p(affinity), _p(scores), _p(out), B, Cc, H, W, arr, len(dil), int(num_iter), _p(ws),
                                    ws.numel(), _stream()))
    return out


def pamr_labels(scores, thresh=0.5, min_conf=0.0, ignore_index=255):
    """Refined scores (B,C,H,W) -> int64 labels (B,H,W), what ``train_step`` takes as masks.  C >= 2: the first maximum's
    index, ``ignore_index`` where that maximum is below ``min_conf``; C == 1: ``scores >= thresh``.  On the device."""
    if not torch.is_tensor(scores) or scores.dim() != 4:
        raise WsdlError("pamr_labels: scores must be a (B,C,H,W) tensor")
    scores = _dense(scores.detach(), "pamr_labels: scores")
    B, Cc, H, W = scores.shape
    labels = torch.empty(B, H, W, device=scores.device, dtype=torch.int64)
    check(lib().wsdl_pamr_labels(_p(scores), B, Cc, H, W, float(thresh), float(min_conf), int(ignore_index), _p(labels), _stream()))
    return labels


# ---- multi-scale + flip test-time fusion (csrc/multiscale.hip; include/wsdl_hip.h "multi-scale fusion")
MS_MAX_SOURCES = 8
MS_MAX_CHANNELS = 64
_MS_ACTIVATIONS = {"none": 0, "softmax": 1, "sigmoid": 2}
_MS_REDUCTIONS = {"mean": 0, "max": 1}


class _MsSource(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("weight", C.c_float), ("mirrored", C.c_int)]


def _hw(size, name):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: size {size!r} must be (H, W)") from None
    if H < 1 or W < 1:
        raise ValueError(f"{name}: size {size!r} must be positive")
    return H, W


def multiscale_sizes(H, W, scales, multiple=32):
    """The input sizes of a multi-scale pass over H x W images: per scale ``s`` the pair
    ``(max(multiple, floor(s H / multiple + 0.5) multiple), likewise for W)`` - the nearest multiple, halves up, never below one
    ``multiple`` (the networks' output stride is 8 and the classifier's 32).  Host only.  ValueError for a scale that is not a
    positive finite number, for more than 8 scales, for none, and for two scales that land on the same size."""
    if isinstance(multiple, bool) or not isinstance(multiple, int) or multiple < 1:
        raise ValueError(f"multiscale_sizes: multiple {multiple!r} must be an int >= 1")
    H, W = _hw((H, W), "multiscale_sizes")
    try:
        scales = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise ValueError(f"multiscale_sizes: scales {scales!r} must be a sequence of numbers") from None
    if not 1 <= len(scales) <= MS_MAX_SOURCES:
        raise ValueError(f"multiscale_sizes: 1 to {MS_MAX_SOURCES} scales, got {len(scales)}")
    if any(not (s > 0 and s < float("inf")) for s in scales):
        raise ValueError(f"multiscale_sizes: scales {scales!r} must be positive and finite")
    sizes = [(max(multiple, int(np.floor(s * H / multiple + 0.5)) * multiple), max(multiple, int(np.floor(s * W / multiple + 0.5)) * multiple))
             for s in scales]
    if len(set(sizes)) != len(sizes):
        raise ValueError(f"multiscale_sizes: scales {scales!r} give the sizes {sizes!r}: two scales land on the same size")
    return sizes


def scale_flip(images, size, flip=False, out=None):
    """images (B,C,H,W) float32 on the device -> ((1 + flip) B, C, h, w): images ``[0, B)`` are ``bilinear_resize(images, size)``
    bit for bit (a copy when ``size`` is the input's), images ``[B, 2B)`` the same planes mirrored left-right - resize, THEN
    mirror (mirror-then-resize differs in the last bit).  One launch, no host read, not differentiable (the input is detached);
    a launch plan can hold the call.  A strided input is copied first.  ``out``: a dense float32 tensor of the result's shape on
    the same device that receives it (it must not overlap ``images``)."""
    h, w = _hw(size, "scale_flip")
    if not torch.is_tensor(images) or images.dim() != 4 or images.numel() == 0:
        raise WsdlError("scale_flip: images must be a non-empty (B,C,H,W) tensor")
    images = _dense(images.detach(), "scale_flip: images")
    B, Cc, H, W = images.shape
    shape = (B * (2 if flip else 1), Cc, h, w)
    if out is None:
        out = torch.empty(shape, device=images.device, dtype=torch.float32)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.device == images.device and out.is_contiguous() and not out.requires_grad):
        raise WsdlError(f"scale_flip: out must be a dense float32 {shape} tensor on {images.device} that needs no gradient")
    check(lib().wsdl_scale_flip(_p(images), _p(out), B, Cc, H, W, h, w, int(bool(flip)), _stream()))
    return out


def check_multiscale_fuse(sources, size, mirrored=False, weights=None, activation="none", reduce="mean"):
    """The host-side refusals of ``multiscale_fuse`` - before any device work, each stating its cause.  Returns
    ``(B, C, H, W, mirrored flags, weights)``."""
    H, W = _hw(size, "multiscale_fuse")
    if activation not in _MS_ACTIVATIONS:
        raise ValueError(f"multiscale_fuse: activation {activation!r}: 'none', 'softmax' or 'sigmoid'")
    if reduce not in _MS_REDUCTIONS:
        raise ValueError(f"multiscale_fuse: reduce {reduce!r}: 'mean' or 'max'")
    if torch.is_tensor(sources):
        sources = [sources]
    sources = list(sources)
    n = len(sources)
    if not 1 <= n <= MS_MAX_SOURCES:
        raise ValueError(f"multiscale_fuse: 1 to {MS_MAX_SOURCES} sources, got {n}")
    if isinstance(mirrored, (bool, int)):
        mirrored = [bool(mirrored)] * n
    else:
        mirrored = [bool(m) for m in mirrored]
        if len(mirrored) != n:
            raise ValueError(f"multiscale_fuse: {len(mirrored)} mirrored flags for {n} sources")
    if weights is not None:
        if reduce == "max":
            raise ValueError("multiscale_fuse: reduce='max' takes no weights")
        try:
            weights = [float(v) for v in weights]
        except (TypeError, ValueError):
            raise ValueError(f"multiscale_fuse: weights {weights!r} must be a sequence of numbers") from None
        if len(weights) != n:
            raise ValueError(f"multiscale_fuse: {len(weights)} weights for {n} sources")
        if any(not (0.0 <= v < float("inf")) for v in weights) or not sum(weights) > 0:
            raise ValueError(f"multiscale_fuse: weights {weights!r} must be finite, >= 0 and not all zero")
    else:
        weights = [1.0] * n
    B = Cc = None
    for k, (t, m) in enumerate(zip(sources, mirrored)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.numel() == 0:
            raise WsdlError(f"multiscale_fuse: source {k} must be a non-empty (B,C,h,w) tensor")
        if t.dtype != torch.float32:
            raise WsdlError(f"multiscale_fuse: source {k}: expected torch.float32, got {t.dtype}")
        lead = t.shape[0]
        if m:
            if lead % 2:
                raise WsdlError(f"multiscale_fuse: source {k} is mirrored but its leading dimension {lead} is odd "
                                "(plain images first, then their mirror images)")
            lead //= 2
        if B is None:
            B, Cc = lead, t.shape[1]
        if lead != B:
            raise WsdlError(f"multiscale_fuse: source {k} holds {lead} images, source 0 holds {B}")
        if t.shape[1] != Cc:
            raise WsdlError(f"multiscale_fuse: source {k} has {t.shape[1]} channels, source 0 has {Cc}")
    if Cc > MS_MAX_CHANNELS:
        raise WsdlError(f"multiscale_fuse: {Cc} channels, at most {MS_MAX_CHANNELS}")
    if activation == "softmax" and Cc == 1:
        raise ValueError("multiscale_fuse: activation='softmax' needs more than one channel (use 'sigmoid')")
    for k, t in enumerate(sources):
        if not t.is_cuda:
            raise WsdlError(f"multiscale_fuse: source {k}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if t.device != sources[0].device:
            raise WsdlError(f"multiscale_fuse: source {k} is on {t.device}, source 0 on {sources[0].device}")
    return B, Cc, H, W, mirrored, weights


def multiscale_fuse(sources, size, *, mirrored=False, weights=None, activation="none", reduce="mean", scores=True, labels=False,
                    conf=False, thresh=0.5, min_conf=0.0, ignore_index=255, out=None):
    """Fuse up to 8 float32 device maps of different sizes into one map of ``size`` = (H, W) in ONE launch, without a full-size
    intermediate per source.  ``sources[k]`` is (B,C,h_k,w_k), or (2B,C,h_k,w_k) when ``mirrored`` (a bool for all, or one per
    source): images ``[B, 2B)`` are then the network's outputs for the mirrored inputs, as ``scale_flip(flip=True)`` orders them.
    Every member - a source's plain half, then its mirrored half, in source order - contributes
    ``act(bilinear_resize(member, size))`` at the output pixel, the mirrored half un-mirrored after its resize; a source that
    already has the target's size is read directly.  ``activation``: 'none', 'softmax' (over C, taken AFTER the resize, at the
    output pixel) or 'sigmoid'; ``reduce``: 'mean' (weighted by ``weights``, one per source, default all 1; both halves of a
    source carry its weight) or 'max'.  The members of a pixel are combined in double and rounded once; no atomics: two calls
    give the same bits.

    Returns what was asked for, in this order, as one tensor or a tuple: ``scores`` (B,C,H,W) float32; ``labels`` (B,H,W) int64,
    exactly ``pamr_labels(scores, thresh, min_conf, ignore_index)``; ``conf`` (B,H,W) float32, the score behind the label (C = 1:
    the score).  Labels and ``conf`` need no score planes.  ``out``: a dict whose 'scores' / 'labels' / 'conf' entries, where they
    are dense tensors of the right shape, type and device, receive the results (others are put there).

    Not differentiable (inputs detached), no host read: a launch plan can hold the call.  Strided sources are copied first.
    Refused before any device work, with the cause: a wrong dtype or device, batch / channel / count mismatches, a mirrored source
    with an odd leading dimension, C > 64, more than 8 sources, ``reduce='max'`` with weights, ``activation='softmax'`` with C = 1."""
    B, Cc, H, W, mirrored, weights = check_multiscale_fuse(sources, size, mirrored, weights, activation, reduce)
    if not (scores or labels or conf):
        raise ValueError("multiscale_fuse: nothing asked for (scores, labels, conf)")
    if out is not None and not isinstance(out, dict):
        raise ValueError("multiscale_fuse: out is a dict with 'scores', 'labels' and / or 'conf'")
    if torch.is_tensor(sources):
        sources = [sources]
    srcs = [_dense(t.detach(), "multiscale_fuse: source") for t in sources]
    dev = srcs[0].device
    arr = (_MsSource * len(srcs))()
    for k, (t, m, wt) in enumerate(zip(srcs, mirrored, weights)):
        arr[k].data, arr[k].h, arr[k].w, arr[k].weight, arr[k].mirrored = _p(t), t.shape[2], t.shape[3], wt, int(m)
    t_scores = _out_tensor(out, "scores", (B, Cc, H, W), torch.float32, dev) if scores else None
    t_labels = _out_tensor(out, "labels", (B, H, W), torch.int64, dev) if labels else None
    t_conf = _out_tensor(out, "conf", (B, H, W), torch.float32, dev) if conf else None
    check(lib().wsdl_multiscale_fuse(arr, len(srcs), B, Cc, H, W, _MS_ACTIVATIONS[activation], _MS_REDUCTIONS[reduce], _p(t_scores),
                                     _p(t_labels), _p(t_conf), float(thresh), float(min_conf), int(ignore_index), _stream()))
    res = tuple(t for t in (t_scores, t_labels, t_conf) if t is not None)
    return res[0] if len(res) == 1 else res


def max_normalize(scores, thresh=None, out=None):
    """Divide every image of float32 device ``scores`` (B, ...) by its own maximum - PSA's normalisation of a combined CAM -
    ``v / max`` formed in double and rounded once.  An image whose maximum is <= 0 or not finite (any NaN in it) is left as it
    is.  ``thresh``: also return a uint8 mask of the same shape, ``v >= thresh and v > 0`` on the normalised values (the rule of
    the LayerCAM epilogue's mask).  ``out``: the tensor that receives the result (dense, same shape; may be ``scores`` itself).
    A memset and two launches, the maximum through an integer atomic max: bitwise reproducible, no host read, not
    differentiable; a launch plan can hold the call."""
    if not torch.is_tensor(scores) or scores.dim() < 2 or scores.numel() == 0:
        raise WsdlError("max_normalize: scores must be a non-empty (B, ...) tensor")
    if thresh is not None and not float(thresh) == float(thresh):
        raise ValueError("max_normalize: thresh is NaN")
    x = _dense(scores.detach(), "max_normalize: scores")
    B = x.shape[0]
    if out is None:
        out = torch.empty_like(x)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.device == x.device
              and out.is_contiguous() and not out.requires_grad):
        raise WsdlError(f"max_normalize: out must be a dense float32 {tuple(x.shape)} tensor on {x.device} that needs no gradient")
    nbytes = lib().wsdl_plane_max_workspace(B)
    if nbytes == 0:
        raise WsdlError(f"max_normalize: {B} images, at most 65535")
    mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8) if thresh is not None else None
    ws = workspace(nbytes, x.device)
    check(lib().wsdl_plane_max_normalize(_p(x), _p(out), _p(mask), B, x.numel() // B, float(thresh if thresh is not None else 0.0),
                                         _p(ws), ws.numel(), _stream()))
    return out if mask is None else (out, mask)


# ---- AffinityNet: learned pairwise affinities, their loss, the CAM random walk (csrc/affinity.hip; include/wsdl_hip.h "AffinityNet")
AFFINITY_WEIGHTS = (0.25, 0.25, 0.5)


def affinity_offsets(radius):
    """PSA's half disc of pair offsets ``(dy, dx)`` for ``radius`` in [2, 8], in the order of the affinity planes: first (0,x)
    for x = 1..r-1, then, for y = 1..r-1, every (y,x) with x = -(r-1)..r-1 and x^2 + y^2 < r^2 (4 pairs at r = 2, 34 at r = 5).
    Host only."""
    r = _affinity_radius(radius)
    out = [(0, x) for x in range(1, r)]
    out += [(y, x) for y in range(1, r) for x in range(-(r - 1), r) if x * x + y * y < r * r]
    return out


def _affinity_radius(radius, name="affinity"):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 2 <= radius <= 8:
        raise WsdlError(f"{name}: radius {radius!r} must be an int in [2, 8]")
    return radius


def check_affinity_options(radius=5, *, feat=None, labels=None, aff=None, trans=None, scores=None, out=None, beta=None,
                           num_iter=None, weights=None, eps=None, name="affinity"):
    """Host-side validation of the affinity ops, before any device call: WsdlError for a radius outside [2, 8], a ``beta`` that
    is not a finite number > 0, a ``num_iter`` that is not an int >= 0, ``weights`` that are not three finite numbers, an ``eps``
    that is not > 0, tensors of the wrong rank, type or place, sizes that do not match each other (``labels`` (B,h,w) int64,
    ``aff`` (B,P,h,w), ``trans`` (B,2P+1,h,w), ``scores`` (B,C,h,w) with C <= 32 against ``feat`` (B,D,h,w) with D <= 1024, h w <=
    2^20), and an ``out`` that is not a dense float32 tensor of the expected shape or that shares memory with an input.
    Returns the number of pairs P."""
    r = _affinity_radius(radius, name)
    P = len(affinity_offsets(r))
    if beta is not None and (not _finite_number(beta) or beta <= 0):
        raise WsdlError(f"{name}: beta {beta!r} must be a finite number > 0")
    if num_iter is not None and (isinstance(num_iter, bool) or not isinstance(num_iter, int) or num_iter < 0):
        raise WsdlError(f"{name}: num_iter {num_iter!r} must be an int >= 0")
    if weights is not None:
        try:
            ok = len(weights) == 3 and all(_finite_number(v) for v in weights)
        except TypeError:
            ok = False
        if not ok:
            raise WsdlError(f"{name}: weights {weights!r} must be three finite numbers (bg, fg, neg)")
    if eps is not None and (not _finite_number(eps) or eps <= 0):
        raise WsdlError(f"{name}: eps {eps!r} must be a finite number > 0")
    geom = None                                                     # (B, h, w, device) the tensors must agree on
    for t, what, chan, dtype in ((feat, "feat", None, torch.float32), (labels, "labels", -1, torch.int64), (aff, "aff", P, torch.float32),
                                 (trans, "trans", 2 * P + 1, torch.float32), (scores, "scores", None, torch.float32)):
        if t is None:
            continue
        rank = 3 if chan == -1 else 4
        if not torch.is_tensor(t) or t.dim() != rank:
            raise WsdlError(f"{name}: {what} must be a {'(B,h,w)' if rank == 3 else '(B,C,h,w)'} tensor")
        if t.dtype != dtype:
            raise WsdlError(f"{name}: {what} must be {dtype}, got {t.dtype}")
        if t.numel() == 0:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
        if rank == 4 and chan is not None and t.shape[1] != chan:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} must have {chan} planes at radius {r}")
        if what == "feat" and t.shape[1] > 1024:
            raise WsdlError(f"{name}: feat {tuple(t.shape)}: at most 1024 channels")
        if what == "scores" and t.shape[1] > 32:
            raise WsdlError(f"{name}: scores {tuple(t.shape)}: at most 32 channels")
        g = (t.shape[0], t.shape[-2], t.shape[-1], t.device)
        if g[1] * g[2] > 1 << 20:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)}: h w must be at most 2^20")
        if geom is None:
            geom = g
        elif g != geom:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} on {t.device} does not match the other tensors: batch {geom[0]}, size "
                            f"{geom[1]} x {geom[2]} on {geom[3]}")
    if out is not None:
        if geom is None:
            raise WsdlError(f"{name}: out= needs the tensor it belongs to (scores, or aff for the transitions)")
        like = scores if scores is not None else None
        shape = tuple(like.shape) if like is not None else (geom[0], 2 * P + 1, geom[1], geom[2])
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and out.device == geom[3]
                and out.is_contiguous() and not out.requires_grad):
            raise WsdlError(f"{name}: out must be a dense float32 {shape} tensor on {geom[3]} that needs no gradient")
        for t, what in ((scores, "scores"), (trans, "trans"), (aff, "aff")):
            if t is not None and _shares_memory(out, t):
                raise WsdlError(f"{name}: out shares memory with {what}")
    return P


def _shares_memory(a, b):
    if a.device != b.device or a.numel() == 0 or b.numel() == 0:
        return False
    sa, sb = a.untyped_storage(), b.untyped_storage()
    if sa.data_ptr() != sb.data_ptr():
        return False

    def span(t):
        lo = t.storage_offset()
        hi = lo + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1
        return lo * t.element_size(), hi * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def affinity_workspace(B, D, C_, H, W, radius=5):
    """Bytes of scratch the affinity ops need at this geometry; 0 outside the limits (host-side)."""
    try:
        _affinity_radius(radius)
    except WsdlError:
        return 0
    return int(lib().wsdl_affinity_workspace(int(B), int(D), int(C_), int(H), int(W), radius))


def _affinity_ws(name, B, D, C_, H, W, radius, device):
    nbytes = lib().wsdl_affinity_workspace(B, D, C_, H, W, radius)
    if nbytes == 0:
        raise WsdlError(f"{name}: bad geometry B={B} D={D} C={C_} h={H} w={W} radius={radius}")
    return workspace(nbytes, device)


class _PairAffinity(torch.autograd.Function):
    """wsdl_affinity_pair_affinity / _backward: one launch each."""

    @staticmethod
    def forward(ctx, feat, radius, P):
        feat = _dense(feat, "pair_affinity: feat")
        B, D, H, W = feat.shape
        aff = torch.empty(B, P, H, W, device=feat.device, dtype=torch.float32)
        check(lib().wsdl_affinity_pair_affinity(_p(feat), B, D, H, W, radius, _p(aff), _stream()))
        ctx.radius = radius
        ctx.save_for_backward(feat, aff)
        return aff

    @staticmethod
    def backward(ctx, daff):
        feat, aff = ctx.saved_tensors
        B, D, H, W = feat.shape
        dfeat = torch.empty_like(feat)
        check(lib().wsdl_affinity_pair_affinity_backward(_p(feat), _p(aff), _p(_dense(daff, "pair_affinity: upstream gradient")),
                                                         _p(dfeat), B, D, H, W, ctx.radius, _stream()))
        return dfeat, None, None


def pair_affinity(feat, radius=5):
    """AffinityNet's pairwise affinities (Ahn & Kwak, CVPR 2018) of float32 device features (B,D,h,w): (B,P,h,w) float32 with
    ``a(p,j) = exp(-mean_d |f_d(p) - f_d(p + o_j)|)`` for the offsets ``o_j`` of ``affinity_offsets(radius)`` and exactly 0 where
    ``p + o_j`` lies outside the image.  Differentiable in ``feat`` (closed-form gather, no atomics); one launch each way,
    bitwise reproducible."""
    P = check_affinity_options(radius, feat=feat, name="pair_affinity")
    _req(feat, "pair_affinity: feat")
    return _PairAffinity.apply(feat, radius, P)


def affinity_pair_counts(labels, radius=5, ignore_index=255):
    """int64 (3,) on the device: the numbers of bg-positive, fg-positive and negative pairs of int64 labels (B,h,w) over the
    half disc of ``radius`` - both ends != ``ignore_index`` and equal 0 / equal > 0 / different; exact, no host read."""
    check_affinity_options(radius, labels=labels, name="affinity_pair_counts")
    _req(labels, "affinity_pair_counts: labels", torch.int64)
    labels = labels.contiguous()
    B, H, W = labels.shape
    counts = torch.empty(3, device=labels.device, dtype=torch.int64)
    ws = _affinity_ws("affinity_pair_counts", B, 1, 1, H, W, radius, labels.device)
    check(lib().wsdl_affinity_pair_counts(_p(labels), B, H, W, radius, int(ignore_index), _p(counts), _p(ws), ws.numel(), _stream()))
    return counts


class _AffinityLoss(torch.autograd.Function):
    """wsdl_affinity_loss: the loss and its complete gradient in five launches; the backward multiplies by the upstream
    gradient only."""

    @staticmethod
    def forward(ctx, feat, labels, radius, ignore_index, weights, eps):
        feat = _dense(feat, "affinity_loss: feat")
        B, D, H, W = feat.shape
        loss = torch.empty((), device=feat.device, dtype=torch.float32)
        dfeat = torch.empty_like(feat) if ctx.needs_input_grad[0] else None      # (asked of the argument: `feat` may be a dense copy)
        ws = _affinity_ws("affinity_loss", B, D, 1, H, W, radius, feat.device)
        check(lib().wsdl_affinity_loss(_p(feat), _p(labels), _p(loss), _p(dfeat), None, B, D, H, W, radius, ignore_index, weights[0],
                                       weights[1], weights[2], eps, _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dfeat)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dfeat,) = ctx.saved_tensors
        return (_scaled_grad(dfeat, g),) + (None,) * 5


def affinity_loss(feat, labels, *, radius=5, ignore_index=255, weights=AFFINITY_WEIGHTS, eps=1e-5):
    """AffinityNet's training loss (PSA's ``train_aff``) on float32 device features (B,D,h,w) and int64 labels (B,h,w), a 0-dim
    float32 tensor with its gradient.  Pairs over ``affinity_offsets(radius)``; a pair whose ends are both not
    ``ignore_index`` is bg-positive (both 0), fg-positive (equal, > 0) or negative (different), anything else is not counted.
    With the exact counts ``n`` over the batch: ``w_bg sum_bg -log(a + eps) / (n_bg + eps) + w_fg sum_fg -log(a + eps) / (n_fg +
    eps) + w_neg sum_neg -log(1 + eps - a) / (n_neg + eps)``, ``weights = (w_bg, w_fg, w_neg)``.  An empty kind adds 0; without
    a counted pair the loss and its gradient are 0.  Sums in double in a fixed order, no float atomics: bitwise reproducible;
    no host read - a launch plan can hold the call and its backward."""
    check_affinity_options(radius, feat=feat, labels=labels, weights=weights, eps=eps, name="affinity_loss")
    _req(feat, "affinity_loss: feat")
    _req(labels, "affinity_loss: labels", torch.int64)
    return _AffinityLoss.apply(feat, labels.detach().contiguous(), radius, int(ignore_index), tuple(float(v) for v in weights),
                               float(eps))


def affinity_transitions(aff, beta=8.0, radius=5, out=None):
    """The random walk's transition weights from affinities (B,P,h,w): (B,2P+1,h,w) float32 - plane 0 the pixel itself
    (affinity 1), plane 1 + 2j its neighbour at offset j, plane 2 + 2j the neighbour at the reversed offset; ``a ** beta`` over
    the sum of the pixel's row (>= 1 by the self term), 0 where the neighbour is outside the image.  Not differentiable."""
    check_affinity_options(radius, aff=aff, out=out, beta=beta, name="affinity_transitions")
    aff = _dense(aff.detach(), "affinity_transitions: aff")
    B, P, H, W = aff.shape
    if out is None:
        out = torch.empty(B, 2 * P + 1, H, W, device=aff.device, dtype=torch.float32)
    _req(out, "affinity_transitions: out")
    check(lib().wsdl_affinity_transitions(_p(aff), _p(out), B, H, W, radius, float(beta), _stream()))
    return out


def random_walk(trans, scores, num_iter, *, radius=5, out=None):
    """``num_iter`` steps ``m'_c(p) = sum_q w(p,q) m_c(q)`` of float32 device scores (B,C,h,w), 1 <= C <= 32, under the weights of
    ``affinity_transitions`` - PSA's ``cam @ T^num_iter`` without the dense matrix.  Every step is a convex combination: the
    result stays inside the input's range and a constant map is a fixed point; ``num_iter=0`` copies.  Not differentiable (the
    inputs are detached); no host read, bitwise reproducible.  ``out``: a dense float32 tensor that receives the result; it
    must not share memory with an input.  One launch per step: a launch plan can hold the call."""
    check_affinity_options(radius, trans=trans, scores=scores, out=out, num_iter=num_iter, name="random_walk")
    trans = _dense(trans.detach(), "random_walk: trans")
    scores = _dense(scores.detach(), "random_walk: scores")
    B, Cc, H, W = scores.shape
    if out is None:
        out = torch.empty_like(scores)
    _req(out, "random_walk: out")
    ws = _affinity_ws("random_walk", B, 1, Cc, H, W, radius, scores.device)
    check(lib().wsdl_affinity_random_walk(_p(trans), _p(scores), _p(out), B, Cc, H, W, radius, num_iter, _p(ws),
                                          ws.numel(), _stream()))
    return out


def affinity_random_walk(feat, scores, *, radius=5, beta=8.0, num_iter=256):
    """``random_walk(affinity_transitions(pair_affinity(feat)), scores)``: scores (B,C,h,w) propagated under the affinities of
    features (B,D,h,w) on the same h x w.  Not differentiable."""
    check_affinity_options(radius, feat=feat, scores=scores, beta=beta, num_iter=num_iter, name="affinity_random_walk")
    trans = affinity_transitions(pair_affinity(feat.detach(), radius), beta, radius)
    return random_walk(trans, scores, num_iter, radius=radius)


# ---- class prototypes, prototype similarity maps, the pixel-to-prototype contrast loss (csrc/prototype.hip; include/wsdl_hip.h
# "Class prototypes")
PROTOTYPE_MAX_CHANNELS, PROTOTYPE_MAX_CLASSES = 2048, 32
_PROTO_ACTIVATIONS = {"none": 0, "relu": 1, "softmax": 2}


def check_prototype_options(*, feat=None, labels=None, proto=None, mass=None, present=None, pixel_weight=None, bank=None, count=None,
                            num_classes=None, temperature=None, eps=None, momentum=None, activation=None, reduction=None, out=None,
                            name="prototype"):
    """Host-side validation of the prototype ops, before any device call.  WsdlError for: a ``num_classes`` that is not an int in
    [1, 32]; a ``temperature`` or an ``eps`` that is not a finite number > 0; a ``momentum`` outside [0, 1]; an unknown
    ``activation`` / ``reduction``; tensors of the wrong rank, type or place - ``feat`` (B,D,h,w) float32 with D <= 2048 and h w <=
    2^20, ``labels`` (B,h,w) int64, ``pixel_weight`` (B,h,w) float32, ``proto`` (S,K,D) float32 with K <= 32, ``mass`` (S,K) float32,
    ``present`` (S,K) bool / uint8, ``bank`` (K,D) float32 and ``count`` (K,) int64; a number of segments S that is neither 1 nor the
    batch size, or that differs between ``proto``, ``mass`` and ``present``; an ``out`` that is not a dense float32 tensor of the
    result's shape (``(B,K,h,w)`` beside ``proto``, else ``(proto (S,K,D), mass (S,K))``), that needs a gradient or that shares
    memory with an input.  Returns ``(K, S)`` (None where unknown)."""
    K = None
    if num_classes is not None:
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= PROTOTYPE_MAX_CLASSES:
            raise WsdlError(f"{name}: num_classes {num_classes!r} must be an int in [1, {PROTOTYPE_MAX_CLASSES}]")
        K = num_classes
    for v, what in ((temperature, "temperature"), (eps, "eps")):
        if v is not None and (not _finite_number(v) or v <= 0):
            raise WsdlError(f"{name}: {what} {v!r} must be a finite number > 0")
    if momentum is not None and (not _finite_number(momentum) or not 0.0 <= momentum <= 1.0):
        raise WsdlError(f"{name}: momentum {momentum!r} must be a number in [0, 1]")
    if activation is not None and activation not in _PROTO_ACTIVATIONS:
        raise WsdlError(f"{name}: activation {activation!r}: 'none', 'relu' or 'softmax'")
    if reduction is not None and reduction not in _CE_REDUCTIONS:
        raise WsdlError(f"{name}: reduction {reduction!r}: 'mean', 'sum' or 'none'")
    tensors = ((feat, "feat", 4, (torch.float32,)), (labels, "labels", 3, (torch.int64,)),
               (pixel_weight, "pixel_weight", 3, (torch.float32,)), (proto, "proto", 3, (torch.float32,)),
               (mass, "mass", 2, (torch.float32,)), (present, "present", 2, (torch.bool, torch.uint8)),
               (bank, "bank", 2, (torch.float32,)), (count, "count", 1, (torch.int64,)))
    for t, what, rank, dtypes in tensors:
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() != rank:
            raise WsdlError(f"{name}: {what} must be a tensor of rank {rank}")
        if t.dtype not in dtypes:
            raise WsdlError(f"{name}: {what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.numel() == 0:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
    B = D = None
    if feat is not None:
        B, D, h, w = feat.shape
        if D > PROTOTYPE_MAX_CHANNELS:
            raise WsdlError(f"{name}: feat {tuple(feat.shape)}: at most {PROTOTYPE_MAX_CHANNELS} channels")
        if h * w > 1 << 20:
            raise WsdlError(f"{name}: feat {tuple(feat.shape)}: h w must be at most 2^20")
        for t, what in ((labels, "labels"), (pixel_weight, "pixel_weight")):
            if t is not None and tuple(t.shape) != (B, h, w):
                raise WsdlError(f"{name}: {what} {tuple(t.shape)} must be {(B, h, w)}, the size of feat {tuple(feat.shape)}")
    S = None
    if proto is not None:
        S, Kp, Dp = proto.shape
        if Kp > PROTOTYPE_MAX_CLASSES:
            raise WsdlError(f"{name}: proto {tuple(proto.shape)}: at most {PROTOTYPE_MAX_CLASSES} classes")
        if K is not None and Kp != K:
            raise WsdlError(f"{name}: proto {tuple(proto.shape)} does not have num_classes = {K} classes")
        K = Kp
        if Dp > PROTOTYPE_MAX_CHANNELS or (D is not None and Dp != D):
            raise WsdlError(f"{name}: proto {tuple(proto.shape)} must have the channels of feat, {D if D is not None else '<= 2048'}")
        D = Dp
        if B is not None and S not in (1, B):
            raise WsdlError(f"{name}: proto {tuple(proto.shape)}: {S} segments for a batch of {B} (1 or the batch size)")
    for t, what in ((mass, "mass"), (present, "present")):
        if t is None:
            continue
        if K is not None and t.shape[1] != K:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} must have {K} classes")
        K = t.shape[1]
        if K > PROTOTYPE_MAX_CLASSES:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)}: at most {PROTOTYPE_MAX_CLASSES} classes")
        if S is not None and t.shape[0] != S:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has {t.shape[0]} segments, the other tensors {S}")
        S = t.shape[0]
        if B is not None and S not in (1, B):
            raise WsdlError(f"{name}: {what} {tuple(t.shape)}: {S} segments for a batch of {B} (1 or the batch size)")
    if bank is not None:
        if bank.shape[0] > PROTOTYPE_MAX_CLASSES or bank.shape[1] > PROTOTYPE_MAX_CHANNELS:
            raise WsdlError(f"{name}: bank {tuple(bank.shape)}: at most {PROTOTYPE_MAX_CLASSES} classes of {PROTOTYPE_MAX_CHANNELS} channels")
        if S is not None and S != 1:
            raise WsdlError(f"{name}: the bank takes the prototypes of one segment, got {S}")
        if (K is not None and bank.shape[0] != K) or (D is not None and bank.shape[1] != D):
            raise WsdlError(f"{name}: bank {tuple(bank.shape)} must be {(K, D)}")
        K, D = bank.shape
        if count is not None and count.shape[0] != K:
            raise WsdlError(f"{name}: count {tuple(count.shape)} must be {(K,)}")
        if not bank.is_contiguous() or (count is not None and not count.is_contiguous()) or bank.requires_grad:
            raise WsdlError(f"{name}: bank and count must be dense and need no gradient")
        if proto is not None and _shares_memory(bank, proto):
            raise WsdlError(f"{name}: bank shares memory with proto")
    if out is not None:
        if feat is None:
            raise WsdlError(f"{name}: out= needs the features it belongs to")
        if proto is not None:
            wanted = [(out, (B, K, feat.shape[2], feat.shape[3]), "out")]
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 2 or K is None:
                raise WsdlError(f"{name}: out must be a pair (proto, mass) of tensors")
            wanted = [(out[0], None, "out[0]"), (out[1], None, "out[1]")]
            if torch.is_tensor(out[0]) and out[0].dim() == 3:
                So = out[0].shape[0]
                wanted = [(out[0], (So, K, D), "out[0]"), (out[1], (So, K), "out[1]")]
        for t, shape, what in wanted:
            if not (torch.is_tensor(t) and shape is not None and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)
                    and t.device == feat.device and t.is_contiguous() and not t.requires_grad):
                raise WsdlError(f"{name}: {what} must be a dense float32 {shape if shape is not None else '(S,K,D)'} tensor on "
                                f"{feat.device} that needs no gradient")
            for other, oname in ((feat, "feat"), (proto, "proto"), (labels, "labels"), (pixel_weight, "pixel_weight"),
                                 (present, "present")):
                if other is not None and _shares_memory(t, other):
                    raise WsdlError(f"{name}: {what} shares memory with {oname}")
        if len(wanted) == 2 and _shares_memory(wanted[0][0], wanted[1][0]):
            raise WsdlError(f"{name}: out[0] shares memory with out[1]")
    device = None                                   # the place last: everything above can be refused without a device
    for t, what, _rank, _dtypes in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise WsdlError(f"{name}: {what}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if device is None:
            device = t.device
        elif t.device != device:
            raise WsdlError(f"{name}: {what} is on {t.device}, the other tensors on {device}")
    return K, S


def prototype_workspace(B, D, K, H, W):
    """Bytes of scratch the prototype ops need at this geometry; 0 outside the limits (host-side)."""
    return int(lib().wsdl_proto_workspace(int(B), int(D), int(K), int(H), int(W)))


def _proto_ws(name, B, D, K, H, W, device):
    nbytes = _ws_bytes("wsdl_proto_workspace", B, D, K, H, W)
    if nbytes == 0:
        raise WsdlError(f"{name}: bad geometry B={B} D={D} K={K} h={H} w={W}")
    return workspace(nbytes, device)


def _present_u8(present):
    if present is None:
        return None
    present = present.detach().contiguous()
    return present.view(torch.uint8) if present.dtype == torch.bool else present


def class_prototypes(feat, labels, num_classes, *, pixel_weight=None, per_image=True, normalize=True, ignore_index=255, eps=1e-12,
                     out=None):
    """Class prototypes of float32 device features (B,D,h,w) under int64 labels (B,h,w): ``(proto, mass)`` with ``proto`` (S,K,D)
    and ``mass`` (S,K) float32, a segment being one image (``per_image``, S = B) or the whole batch (S = 1).  ``mass[s,k]`` is the
    sum of ``pixel_weight`` (B,h,w) float32, or of 1, over the segment's pixels with label k; labels equal to ``ignore_index`` or
    outside [0, K) are not pooled.  ``proto[s,k]`` is the weighted mean over those pixels of the unit vector ``f_p / max(|f_p|,
    eps)`` (``normalize``, the default) or of ``f_p``; exactly 0 where the mass is 0.  Sums in double in a fixed order, no
    atomics: bitwise reproducible; no host read - a launch plan can hold the call.  Not differentiable (the inputs are
    detached).  ``out``: a pair of dense float32 tensors that receive the results; they must not share memory with an input."""
    check_prototype_options(feat=feat, labels=labels, pixel_weight=pixel_weight, num_classes=num_classes, eps=eps, out=out,
                            name="class_prototypes")
    feat = _dense(feat.detach(), "class_prototypes: feat")
    labels = labels.detach().contiguous()
    pixel_weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    B, D, H, W = feat.shape
    S = B if per_image else 1
    if out is None:
        out = (torch.empty(S, num_classes, D, device=feat.device, dtype=torch.float32),
               torch.empty(S, num_classes, device=feat.device, dtype=torch.float32))
    elif out[0].shape[0] != S:
        raise WsdlError(f"class_prototypes: out[0] {tuple(out[0].shape)} must have {S} segments")
    ws = _proto_ws("class_prototypes", B, D, num_classes, H, W, feat.device)
    check(lib().wsdl_proto_pool(_p(feat), _p(labels), _p(pixel_weight), _p(out[0]), _p(out[1]), B, D, H, W, num_classes, int(bool(per_image)),
                                int(bool(normalize)), int(ignore_index), float(eps), _p(ws), ws.numel(), _stream()))
    return out[0], out[1]


def prototype_similarity(feat, proto, *, activation="none", temperature=1.0, present=None, eps=1e-12, out=None):
    """Cosine similarity of every pixel of float32 device features (B,D,h,w) to the prototypes (S,K,D) of its segment (S = 1: the
    same for every image, S = B: its image's): (B,K,h,w) float32, ``<f_p / max(|f_p|, eps), q_k / max(|q_k|, eps)>``, 0 for a zero
    prototype.  ``activation``: 'none', 'relu' (SIPE's prototype CAM) or 'softmax' - over the classes marked in ``present`` (S,K)
    bool / uint8 (None: all) of the similarity over ``temperature``, exactly 0 for an absent class.  One pass over the features;
    not differentiable; no host read, bitwise reproducible.  ``out``: a dense float32 tensor that receives the result."""
    K, S = check_prototype_options(feat=feat, proto=proto, present=present, activation=activation, temperature=temperature, eps=eps,
                                   out=out, name="prototype_similarity")
    feat = _dense(feat.detach(), "prototype_similarity: feat")
    proto = _dense(proto.detach(), "prototype_similarity: proto")
    present = _present_u8(present)
    B, D, H, W = feat.shape
    if out is None:
        out = torch.empty(B, K, H, W, device=feat.device, dtype=torch.float32)
    ws = _proto_ws("prototype_similarity", B, D, K, H, W, feat.device)
    check(lib().wsdl_proto_similarity(_p(feat), _p(proto), _p(present), _p(out), B, D, H, W, K, S, _PROTO_ACTIVATIONS[activation],
                                      float(temperature), float(eps), _p(ws), ws.numel(), _stream()))
    return out


class _PrototypeContrast(torch.autograd.Function):
    """wsdl_proto_contrast: the loss and its gradient in one pass; the backward multiplies by the upstream gradient only."""

    @staticmethod
    def forward(ctx, feat, proto, labels, present, pixel_weight, K, S, ignore_index, temperature, eps, reduction):
        feat = _dense(feat, "prototype_contrast_loss: feat")
        B, D, H, W = feat.shape
        none = reduction == 2
        loss = torch.empty((B, H, W) if none else (), device=feat.device, dtype=torch.float32)
        dfeat = torch.empty_like(feat) if ctx.needs_input_grad[0] else None      # (asked of the argument: `feat` may be a dense copy)
        inv = torch.empty(1, device=feat.device, dtype=torch.float32) if reduction == 0 else None
        ws = _proto_ws("prototype_contrast_loss", B, D, K, H, W, feat.device)
        check(lib().wsdl_proto_contrast(_p(feat), _p(proto), _p(labels), _p(present), _p(pixel_weight), _p(loss), _p(dfeat), _p(inv), B, D, H,
                                        W, K, S, ignore_index, temperature, eps, reduction, _p(ws), ws.numel(), _stream()))
        ctx.none = none
        ctx.save_for_backward(dfeat, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dfeat, inv = ctx.saved_tensors
        if not ctx.none:
            return (_scaled_grad(dfeat, g, inv),) + (None,) * 10
        out = torch.empty_like(dfeat)
        B, D, H, W = dfeat.shape
        check(lib().wsdl_scale_by_pixel(_p(dfeat), _p(_dense(g, "upstream gradient")), _p(out), B, D, H, W, _stream()))
        return (out,) + (None,) * 10


def prototype_contrast_loss(feat, proto, labels, *, temperature=0.1, present=None, pixel_weight=None, ignore_index=255,
                            reduction="mean", eps=1e-12):
    """Pixel-to-prototype contrast (InfoNCE; Du et al., CVPR 2022) of float32 device features (B,D,h,w) against prototypes (S,K,D)
    (S = 1 or B) under int64 labels (B,h,w): with ``z_{p,k} = cos(f_p, q_k) / temperature`` over the classes marked in
    ``present`` (S,K) bool / uint8 (None: all), ``l_p = -log softmax(z_p)[label_p]``.  A pixel counts iff its label is not
    ``ignore_index`` and its class is present; a label outside [0, K) other than ``ignore_index`` gives NaN ('none': at that pixel
    only).  'mean' is ``sum w_p l_p / sum w_p`` over the counted pixels with ``w_p = pixel_weight`` (B,h,w) float32 or 1, and 0 -
    with a zero gradient - when no pixel counts; 'sum' and 'none' as in ``cross_entropy``.  The gradient flows into ``feat``
    only (the prototypes are constants, as in the papers) and comes from the same launch; an uncounted pixel gets exact zeros.
    Sums in double in a fixed order: bitwise reproducible; no host read - a launch plan can hold the call and its backward."""
    K, S = check_prototype_options(feat=feat, proto=proto, labels=labels, present=present, pixel_weight=pixel_weight,
                                   temperature=temperature, eps=eps, reduction=reduction, name="prototype_contrast_loss")
    pixel_weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    return _PrototypeContrast.apply(feat, _dense(proto.detach(), "prototype_contrast_loss: proto"), labels.detach().contiguous(),
                                    _present_u8(present), pixel_weight, K, S, int(ignore_index), float(temperature), float(eps),
                                    _CE_REDUCTIONS[reduction])


def prototype_ema_(bank, count, proto, mass, momentum):
    """In place: ``bank[k] = momentum bank[k] + (1 - momentum) proto[k]`` and ``count[k] += 1`` for the classes with ``mass[k] >
    0``; a class whose count was 0 takes ``proto[k]`` as it is, a class of zero mass is untouched.  ``bank`` (K,D) float32, ``count``
    (K,) int64, ``proto`` (1,K,D) or (K,D), ``mass`` (1,K) or (K,).  One launch, no host read.  Returns ``bank``."""
    if torch.is_tensor(proto) and proto.dim() == 2:
        proto = proto[None]
    if torch.is_tensor(mass) and mass.dim() == 1:
        mass = mass[None]
    check_prototype_options(proto=proto, mass=mass, bank=bank, count=count, momentum=momentum, name="prototype_ema_")
    if count is None:
        raise WsdlError("prototype_ema_: count must be a (K,) int64 tensor")
    K, D = bank.shape
    check(lib().wsdl_proto_ema(_p(bank), _p(count), _p(_dense(proto.detach(), "prototype_ema_: proto")),
                               _p(_dense(mass.detach(), "prototype_ema_: mass")), K, D, float(momentum), _stream()))
    return bank


# ---- IRN boundary paths: affinities along the line between two pixels, their loss, the boundary CAM walk
# (csrc/boundary_affinity.hip; include/wsdl_hip.h "IRN boundary paths")
def affinity_paths(radius):
    """The path of every offset of ``affinity_offsets(radius)``, in the same order: a list of lists of ``(dy, dx)`` - every
    integer point of the rectangle between (0,0) and the offset whose distance to the line between them is below 1 (IRN's
    thick line), in raster order; both ends are members.  Host only: the table comes from the library, no device is touched."""
    r = _affinity_radius(radius, "affinity_paths")
    P = len(affinity_offsets(r))
    total = lib().wsdl_path_affinity_paths(r, None, None)
    lengths, points = (C.c_int * P)(), (C.c_int * (2 * total))()
    if lib().wsdl_path_affinity_paths(r, lengths, points) != total:
        raise WsdlError(f"affinity_paths: the library has no path table for radius {r}")
    out, at = [], 0
    for n in lengths:
        out.append([(points[2 * s], points[2 * s + 1]) for s in range(at, at + n)])
        at += n
    return out


def _edge_plane(edge, name, what="edge"):
    """The (B,h,w) view of a boundary map given as (B,h,w) or (B,1,h,w); WsdlError for anything else (host-side)."""
    if not torch.is_tensor(edge) or edge.dim() not in (3, 4) or (edge.dim() == 4 and edge.shape[1] != 1):
        raise WsdlError(f"{name}: {what} must be a (B,h,w) or (B,1,h,w) tensor")
    if edge.dtype != torch.float32:
        raise WsdlError(f"{name}: {what} must be torch.float32, got {edge.dtype}")
    if edge.numel() == 0:
        raise WsdlError(f"{name}: {what} {tuple(edge.shape)} has an empty dimension")
    return edge[:, 0] if edge.dim() == 4 else edge


def check_path_affinity_options(radius=5, *, edge=None, labels=None, scores=None, out=None, beta=None, num_iter=None, weights=None,
                                eps=None, name="path_affinity"):
    """Host-side validation of the boundary-path ops, before any device call - ``check_affinity_options`` with a boundary map
    (or its logits) ``edge`` (B,h,w) or (B,1,h,w) float32 in place of the features: WsdlError for a bad radius, beta, num_iter,
    weights or eps, for tensors of the wrong rank, type or place, for ``labels`` (B,h,w) int64 or ``scores`` (B,C,h,w), C <= 32,
    that do not match the map's batch, size (h w <= 2^20) and device, and for an ``out`` that is not a dense float32 tensor of
    the scores' shape or that shares memory with the scores or the map.  Returns the number of pairs P."""
    plane = None if edge is None else _edge_plane(edge, name)[:, None]
    P = check_affinity_options(radius, feat=plane, labels=labels, scores=scores, out=out, beta=beta, num_iter=num_iter, weights=weights,
                               eps=eps, name=name)
    if out is not None and plane is not None and _shares_memory(out, plane):
        raise WsdlError(f"{name}: out shares memory with edge")
    return P


def _path_affinity_ws(name, B, H, W, radius, device):
    nbytes = lib().wsdl_path_affinity_workspace(B, H, W, radius)
    if nbytes == 0:
        raise WsdlError(f"{name}: bad geometry B={B} h={H} w={W} radius={radius}")
    return workspace(nbytes, device)


class _PathAffinity(torch.autograd.Function):
    """wsdl_path_affinity / _backward: one launch each; the arg indices are what the backward needs."""

    @staticmethod
    def forward(ctx, edge, radius, P):
        edge = _dense(edge, "path_affinity: edge")
        B, H, W = edge.shape
        aff = torch.empty(B, P, H, W, device=edge.device, dtype=torch.float32)
        arg = torch.empty(B, P, H, W, device=edge.device, dtype=torch.uint8)
        check(lib().wsdl_path_affinity(_p(edge), B, H, W, radius, _p(aff), _p(arg), _stream()))
        ctx.radius = radius
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return aff, arg

    @staticmethod
    def backward(ctx, daff, _darg):
        (arg,) = ctx.saved_tensors
        B, P, H, W = arg.shape
        dedge = torch.empty(B, H, W, device=arg.device, dtype=torch.float32)
        check(lib().wsdl_path_affinity_backward(_p(_dense(daff, "path_affinity: upstream gradient")), _p(arg), _p(dedge), B, H, W,
                                                ctx.radius, _stream()))
        return dedge, None, None


def path_affinity(edge, radius=5, *, return_arg=False):
    """IRN's boundary-path affinities (Ahn, Cho & Kwak, CVPR 2019) of a float32 device boundary map (B,h,w) or (B,1,h,w) in
    [0, 1]: (B,P,h,w) float32 with ``a(p,j) = 1 - max of edge over the path`` between ``p`` and ``p + o_j``
    (``affinity_paths(radius)``), one float subtraction, and exactly 0 where ``p + o_j`` lies outside the image.  A NaN on the
    path gives NaN.  Differentiable in ``edge``: the gradient of a pair goes to the first point of its path that attains the
    maximum (gather form, no atomics); one launch each way, bitwise reproducible.  ``return_arg``: also the uint8 (B,P,h,w)
    index of that point in its path."""
    P = check_path_affinity_options(radius, edge=edge, name="path_affinity")
    _req(edge, "path_affinity: edge")
    plane = _edge_plane(edge, "path_affinity")
    if return_arg or (plane.requires_grad and torch.is_grad_enabled()):
        aff, arg = _PathAffinity.apply(plane, radius, P)
        return (aff, arg) if return_arg else aff
    plane = _dense(plane.detach(), "path_affinity: edge")
    B, H, W = plane.shape
    aff = torch.empty(B, P, H, W, device=plane.device, dtype=torch.float32)
    check(lib().wsdl_path_affinity(_p(plane), B, H, W, radius, _p(aff), None, _stream()))
    return aff


class _PathAffinityLoss(torch.autograd.Function):
    """wsdl_path_affinity_loss: the loss and its complete gradient in five launches; the backward multiplies by the upstream
    gradient only."""

    @staticmethod
    def forward(ctx, logits, labels, radius, ignore_index, weights, eps, counts_out):
        logits = _dense(logits, "path_affinity_loss: edge_logits")
        B, H, W = logits.shape
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dz = torch.empty_like(logits) if ctx.needs_input_grad[0] else None    # (asked of the argument: `logits` may be a dense copy)
        ws = _path_affinity_ws("path_affinity_loss", B, H, W, radius, logits.device)
        check(lib().wsdl_path_affinity_loss(_p(logits), _p(labels), _p(loss), _p(dz), _p(counts_out), B, H, W, radius, ignore_index,
                                            weights[0], weights[1], weights[2], eps, _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return (_scaled_grad(dz, g),) + (None,) * 6


def path_affinity_loss(edge_logits, labels, *, radius=5, ignore_index=255, weights=AFFINITY_WEIGHTS, eps=1e-5, counts_out=None):
    """IRN's boundary loss (``pos_aff_loss`` / ``neg_aff_loss``) on the float32 device logits (B,h,w) or (B,1,h,w) of a boundary
    head and int64 labels (B,h,w), a 0-dim float32 tensor with its gradient.  Pair kinds and exact counts ``n`` as in
    ``affinity_loss``; with ``zmax`` the largest logit on a pair's path, ``a = sigmoid(-zmax)`` its affinity:
    ``w_bg sum_bg -log(a + eps) / (n_bg + eps) + w_fg sum_fg -log(a + eps) / (n_fg + eps) + w_neg sum_neg -log(sigmoid(zmax) +
    eps) / (n_neg + eps)`` - both sigmoids formed directly in double, so logits of +-40 stay finite.  The gradient of a pair goes
    to the pixel that holds ``zmax``.  An empty kind adds 0; without a counted pair the loss and its gradient are 0.  Sums in
    double in a fixed order, no float atomics: bitwise reproducible; no host read - a launch plan can hold the call and its
    backward.  ``counts_out``: a dense int64 (3,) device tensor that receives the numbers of bg-positive, fg-positive and negative
    pairs the call counted."""
    check_path_affinity_options(radius, edge=edge_logits, labels=labels, weights=weights, eps=eps, name="path_affinity_loss")
    _req(edge_logits, "path_affinity_loss: edge_logits")
    _req(labels, "path_affinity_loss: labels", torch.int64)
    if counts_out is not None:
        if not (torch.is_tensor(counts_out) and counts_out.dtype == torch.int64 and tuple(counts_out.shape) == (3,)
                and counts_out.is_contiguous() and counts_out.device == labels.device):
            raise WsdlError(f"path_affinity_loss: counts_out must be a dense int64 (3,) tensor on {labels.device}")
    return _PathAffinityLoss.apply(_edge_plane(edge_logits, "path_affinity_loss", "edge_logits"), labels.detach().contiguous(), radius,
                                   int(ignore_index), tuple(float(v) for v in weights), float(eps), counts_out)


def edge_random_walk(edge, scores, *, radius=5, beta=10.0, num_iter=256, out=None):
    """IRN's ``propagate_to_edge``: ``random_walk(affinity_transitions(path_affinity(edge), beta), scores * (1 - edge))`` for a
    float32 device boundary map (B,h,w) or (B,1,h,w) and scores (B,C,h,w), 1 <= C <= 32, on the same h x w - the seed is damped on
    predicted boundaries, then walked ``num_iter`` steps on the stencil; a pair whose path crosses a boundary of 1 has affinity 0
    and carries nothing.  Not differentiable; no host read: a launch plan can hold the call.  ``out``: a dense float32 tensor
    that receives the result; it must not share memory with an input."""
    check_path_affinity_options(radius, edge=edge, scores=scores, out=out, beta=beta, num_iter=num_iter, name="edge_random_walk")
    _req(edge, "edge_random_walk: edge")
    plane = _dense(_edge_plane(edge, "edge_random_walk").detach(), "edge_random_walk: edge")
    scores = _dense(scores.detach(), "edge_random_walk: scores")
    B, Cc, H, W = scores.shape
    seed = torch.empty_like(scores)
    check(lib().wsdl_path_affinity_seed(_p(plane), _p(scores), _p(seed), B, Cc, H, W, _stream()))
    trans = affinity_transitions(path_affinity(plane, radius), beta, radius)
    return random_walk(trans, seed, num_iter, radius=radius, out=out)


EDT_FAR = 1 << 30                      # WSDL_EDT_FAR: "no site" in a distance plane
_EDT_METRICS = {"euclid": 0, "chebyshev": 1}


def _edt_labels(labels, name):
    """(B,H,W) int64 device labels; a bool / uint8 mask is converted."""
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise WsdlError(f"{name}: labels must be a (B,H,W) tensor")
    if labels.dtype in (torch.bool, torch.uint8):
        if not labels.is_cuda:
            raise WsdlError(f"{name}: the HIP path needs a device tensor (got {labels.device}); there is no CPU fallback")
        labels = labels.to(torch.int64)
    labels = _req(labels, name + ": labels", torch.int64).detach()
    return labels if labels.is_contiguous() else labels.contiguous()


def _int_option(v, name, lo=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or (lo is not None and v < lo):
        raise ValueError(f"{name} {v!r} must be an int" + ("" if lo is None else f" >= {lo}"))
    return int(v)


def edt(labels, value=1, *, metric="euclid", border=False, want=("out", "in"), out=None):
    """Exact squared distance transform of int64 device labels (B,H,W) (a bool / uint8 mask is converted): a pixel is IN
    where ``labels == value`` and OUT elsewhere, void labels included.  Returns ``(d2_out, d2_in)``, int32 (B,H,W):
    ``d2_out`` the squared distance to the nearest OUT pixel (0 on OUT pixels), ``d2_in`` to the nearest IN pixel (0 on IN
    pixels); a plane ``want`` does not name is ``None`` and is not computed.  ``metric``: 'euclid' (dy^2 + dx^2) or
    'chebyshev' (max(|dy|,|dx|)^2, the distance iterated 3 x 3 erosion measures).  ``border=True``: everything outside the
    image is OUT for ``d2_out``.  ``EDT_FAR`` (2^30) where no site exists.  1 <= H, W <= 8192 (wsdl_edt).

    Two launches, integer arithmetic, no host read, bitwise reproducible: a launch plan can hold the call.  ``out``: a dict
    whose ``"out"`` / ``"in"`` tensors receive the planes (created there when missing or of another shape)."""
    if metric not in _EDT_METRICS:
        raise ValueError(f"edt: metric {metric!r}: 'euclid' or 'chebyshev'")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("out", "in") for w in want):
        raise ValueError(f"edt: want {want!r}: 'out', 'in' or both")
    value = _int_option(value, "edt: value")
    labels = _edt_labels(labels, "edt")
    B, H, W = labels.shape
    planes = [_out_tensor(out, k, (B, H, W), torch.int32, labels.device) if k in want else None for k in ("out", "in")]
    check(lib().wsdl_edt(_p(labels), value, B, H, W, _EDT_METRICS[metric], int(bool(border)), _p(planes[0]), _p(planes[1]),
                         _stream()))
    return tuple(planes)


def _band_limit(width):
    return min(_int_option(width, "boundary band: width", 0) ** 2, 1 << 28)      # every true squared distance is below 2^28


def boundary_band(labels, width, value=1, *, metric="chebyshev", border=True):
    """bool (B,H,W): the IN pixels (``labels == value``) within ``width`` of the contour, ``0 < d2_out <= width^2`` of
    ``edt``.  With the defaults this is the mask minus its ``width``-times 3 x 3-eroded self, the image padded with
    background: the boundary region of Boundary IoU."""
    limit2 = _band_limit(width)
    d, _ = edt(labels, value, metric=metric, border=border, want=("out",))
    return (d > 0) & (d <= limit2)


def boundary_iou_counts(preds, labels, width, value=1, *, metric="chebyshev", border=True, out=None):
    """int64 (B,2) on the device: per image [:, 0] = #(pixels in the boundary bands of both ``preds`` and ``labels``),
    [:, 1] = #(pixels in either) - the bands of ``boundary_band`` (wsdl_band_counts).  No host synchronisation;
    ``boundary_iou_from_counts`` turns a host copy into the metric.  ``out``: a dense int64 (B,2) device tensor to fill."""
    limit2 = _band_limit(width)
    preds, labels = _edt_labels(preds, "boundary_iou_counts"), _edt_labels(labels, "boundary_iou_counts")
    if preds.shape != labels.shape or preds.device != labels.device:
        raise WsdlError(f"boundary_iou_counts: preds {tuple(preds.shape)} on {preds.device} / labels {tuple(labels.shape)} on "
                        f"{labels.device} must match")
    B, H, W = labels.shape
    da, _ = edt(preds, value, metric=metric, border=border, want=("out",))
    db, _ = edt(labels, value, metric=metric, border=border, want=("out",))
    if out is None:
        out = torch.empty((B, 2), device=labels.device, dtype=torch.int64)
    elif not (torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (B, 2) and out.device == labels.device
              and out.is_contiguous()):
        raise WsdlError(f"boundary_iou_counts: out must be a dense int64 {(B, 2)} tensor on {labels.device}")
    check(lib().wsdl_band_counts(_p(da), _p(db), limit2, B, H * W, _p(out), _stream()))
    return out


def boundary_iou_from_counts(counts, EMPTY=1.0):
    """Host arithmetic on (images, 2) counts (anything ``np.asarray`` takes): intersection / union per image as Python
    floats, ``EMPTY`` where the union is 0 (neither mask has a boundary pixel), and the mean over the images as a float in
    [0, 1] (summed in order, as ``iou_from_counts`` does)."""
    rows = np.asarray(counts).reshape(-1, 2).tolist()
    if not rows:
        raise ValueError("boundary_iou_from_counts: no image")
    per = [float(i) / float(u) if u else EMPTY for i, u in rows]
    acc = per[0]
    for v in per[1:]:
        acc += v
    return acc if len(per) == 1 else acc / len(per)


def boundary_width(H, W, ratio=0.02):
    """The band width of the published Boundary IoU: ``max(1, round(ratio * sqrt(H^2 + W^2)))`` pixels."""
    return max(1, int(round(ratio * float(np.sqrt(float(H) ** 2 + float(W) ** 2)))))


def boundary_iou(preds, labels, ratio=0.02, width=None, value=1):
    """Boundary IoU (Cheng et al., CVPR 2021) of int64 (or bool / uint8) device maps (B,H,W), the mean over the images as a
    Python float: per image |Gd and Pd| / |Gd or Pd| with Gd, Pd the pixels of each mask within ``width`` of its contour
    (Chebyshev distance, the image padded with background - the published erosion).  ``width``: pixels, default
    ``boundary_width(H, W, ratio)``.  One host read (the counts)."""
    if width is None:
        if not torch.is_tensor(labels) or labels.dim() != 3:
            raise WsdlError("boundary_iou: labels must be a (B,H,W) tensor")
        width = boundary_width(labels.shape[1], labels.shape[2], ratio)
    return boundary_iou_from_counts(boundary_iou_counts(preds, labels, width, value).cpu().numpy())


def check_boundary_confidence_options(sigma, floor):
    """ValueError for a ``sigma`` that is not a finite number > 0 or a ``floor`` outside [0, 1] (no device needed)."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not 0.0 < sigma < float("inf"):
        raise ValueError(f"boundary_confidence: sigma {sigma!r} must be a finite number > 0")
    if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not 0.0 <= floor <= 1.0:
        raise ValueError(f"boundary_confidence: floor {floor!r} must be a number in [0, 1]")


def boundary_confidence(labels, sigma=3.0, floor=0.0, value=1, *, out=None):
    """float32 (B,H,W) confidence of a label map in its own labels, low at the contour of ``labels == value`` and 1 far from
    it: ``w = floor + (1 - floor) (1 - exp(-d^2 / (2 sigma^2)))`` with ``d`` the Euclidean distance of a pixel to the nearest
    pixel of the other side (``edt`` with ``border=False``: the image edge is no contour); an image without a contour gets
    1 everywhere.  What ``CrossEntropyLoss.set_pixel_weight`` takes: "trust a pseudo label less near its own boundary".
    Three launches, no host read.  ``out``: a dict whose ``"weight"`` (float32) and ``"out"`` / ``"in"`` (int32) tensors
    receive the map and the two distance planes (created there when missing or of another shape)."""
    check_boundary_confidence_options(sigma, floor)
    labels = _edt_labels(labels, "boundary_confidence")
    d_out, d_in = edt(labels, value, out=out if out is not None else {})
    w = _out_tensor(out, "weight", tuple(labels.shape), torch.float32, labels.device)
    check(lib().wsdl_boundary_confidence(_p(d_out), _p(d_in), float(sigma), float(floor), _p(w), w.numel(), _stream()))
    return w


MAX_BOUNDARY_CLASSES = 32              # planes of one signed distance map / classes of one boundary loss


def check_boundary_classes(classes, name="boundary_loss"):
    """ValueError unless ``classes`` is a non-empty tuple (or list) of at most 32 distinct ints >= 0 (no device needed);
    returns it as a tuple of ints."""
    if not isinstance(classes, (tuple, list)) or not 1 <= len(classes) <= MAX_BOUNDARY_CLASSES:
        raise ValueError(f"{name}: classes {classes!r} must be a tuple of 1 to {MAX_BOUNDARY_CLASSES} ints")
    if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0 for c in classes):
        raise ValueError(f"{name}: classes {classes!r} must be ints >= 0")
    classes = tuple(int(c) for c in classes)
    if len(set(classes)) != len(classes):
        raise ValueError(f"{name}: classes {classes!r} must be distinct")
    return classes


_NO_CLASSES = object()


def _logits_labels(name, logits, labels, optional=False, classes=_NO_CLASSES):
    """The front of the losses on (B,C,H,W) logits and (B,H,W) labels -> (labels, classes): logits a 4-d float32 device tensor,
    ``classes`` (where the loss has a list; None = all) against C by ``check_overlap_classes`` - a ValueError, raised before
    anything asks for a device - and labels a (B,H,W) tensor on the logits' device (``optional``: or None), returned detached,
    contiguous and int64."""
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise WsdlError(f"{name}: logits must be a (B,C,H,W) tensor")
    B, Cc, H, W = logits.shape
    if classes is not _NO_CLASSES:
        classes = check_overlap_classes(classes, Cc, name)
    _req(logits, f"{name}: logits")
    if labels is not None or not optional:
        if not torch.is_tensor(labels) or tuple(labels.shape) != (B, H, W) or labels.device != logits.device:
            raise WsdlError(f"{name}: labels must be a {(B, H, W)} tensor on {logits.device}" + (" or None" if optional else ""))
        labels = _req(labels, f"{name}: labels", torch.int64).detach().contiguous()
    return labels, classes


def _device_scalar(name, scale, device):
    """``scale`` of a loss: None, or a one-element float32 tensor on ``device`` (returned detached)."""
    if scale is None:
        return None
    if not torch.is_tensor(scale) or scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != device:
        raise WsdlError(f"{name}: scale must be a one-element float32 tensor on {device} or None")
    return scale.detach()


def signed_distance(labels, value=1, *, out=None):
    """float32 (B,H,W) signed distance map of the class ``labels == value`` (Kervadec et al., MIDL 2019): with the two
    Euclidean planes of ``edt(labels, value, border=False)``, ``phi = +sqrt(d2_in)`` on OUT pixels and ``phi = -(sqrt(d2_out)
    - 1)`` on IN pixels - the published ``distance(negmask) * negmask - (distance(posmask) - 1) * posmask``.  Where the class is
    absent from an image or fills it (a plane holds ``EDT_FAR``), ``phi = 0`` for the whole image: the published "class absent
    -> zeros", extended to the full image, where scipy's transform is undefined.  Void labels are OUT (``edt``'s rule).  The
    root is taken in double and rounded once.  Three launches (wsdl_edt, wsdl_signed_distance), no host read.  ``out``: a dict
    whose ``"phi"`` (float32) and ``"out"`` / ``"in"`` (int32) tensors receive the map and the two planes (created there when
    missing or of another shape)."""
    value = _int_option(value, "signed_distance: value")
    labels = _edt_labels(labels, "signed_distance")
    B, H, W = labels.shape
    d_out, d_in = edt(labels, value, out=out if out is not None else {})
    phi = _out_tensor(out, "phi", (B, H, W), torch.float32, labels.device)
    check(lib().wsdl_signed_distance(_p(d_out), _p(d_in), _p(phi), B, H * W, 0, _stream()))
    return phi


def signed_distance_classes(labels, classes, *, out=None):
    """float32 (B,K,H,W): plane ``k`` is ``signed_distance(labels, classes[k])`` bit for bit - one ``edt`` and one conversion
    per class, written straight into the plane (a multi-value transform is not built).  ``classes``: a non-empty tuple of at
    most 32 distinct ints.  ``out``: a dict whose ``"phi"`` (float32 (B,K,H,W)) and ``"out"`` / ``"in"`` (int32 (B,H,W), the
    planes of the LAST class) tensors are reused."""
    classes = check_boundary_classes(classes, "signed_distance_classes")
    labels = _edt_labels(labels, "signed_distance_classes")
    B, H, W = labels.shape
    K = len(classes)
    bufs = out if out is not None else {}
    phi = _out_tensor(out, "phi", (B, K, H, W), torch.float32, labels.device)
    for k, c in enumerate(classes):
        d_out, d_in = edt(labels, c, out=bufs)
        check(lib().wsdl_signed_distance(_p(d_out), _p(d_in), _p(phi[:, k]), B, H * W, K * H * W, _stream()))
    return phi


class _BoundaryLoss(torch.autograd.Function):
    """wsdl_boundary_loss_fwd_bwd: the loss and its un-normalised gradient in one kernel; the backward multiplies by the
    upstream gradient and the factor scale / (K N) the kernel left on the device (``_scaled_grad``)."""

    @staticmethod
    def forward(ctx, logits, phi, labels, classes, ignore_index, scale):
        logits = _dense(logits, "logits")
        B, Cc, H, W = logits.shape
        K = len(classes)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        need = logits.requires_grad
        dl = torch.empty_like(logits) if need else None
        inv = torch.empty(1, device=logits.device, dtype=torch.float32)
        ws = workspace(lib().wsdl_reduce_workspace(), logits.device)
        cls = (C.c_int * K)(*classes)
        check(lib().wsdl_boundary_loss_fwd_bwd(_p(logits), _p(phi), _p(labels), cls, K, _p(loss), _p(dl), _p(inv), _p(scale),
                                               B, Cc, H, W, int(ignore_index), _p(ws), ws.numel(), _stream()))
        ctx.save_for_backward(dl, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, inv = ctx.saved_tensors
        return _scaled_grad(dl, g, inv), None, None, None, None, None


def boundary_loss(logits, phi, labels=None, *, classes=(1,), ignore_index=-100, scale=None):
    """The boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced segmentation", MIDL 2019) on (B,C,H,W)
    logits: ``scale / (K N) * sum over valid pixels p and the K classes c of softmax(logits)_c(p) * phi_c(p)`` - a 0-dim
    float32 tensor - with its gradient from the same kernel (wsdl_boundary_loss_fwd_bwd).  It moves a contour in proportion to
    its distance from the label's contour; an additive regulariser (``CrossEntropyBoundaryLoss``), negative where the
    prediction sits inside the label.

    ``phi``: float32 (B,K,H,W) signed distance maps, plane ``k`` belonging to class ``classes[k]`` (``signed_distance_classes``),
    or (B,H,W) when ``K == 1`` - a constant, so a caller may compute it once per dataset.  ``labels`` (B,H,W) int64 or None
    only say which pixels count: those with ``labels != ignore_index`` (None: all), ``N`` of them; ``N == 0`` gives 0 with a zero
    gradient, not NaN.  ``scale``: a one-element float32 device tensor (a weight that changes without a new launch plan) or
    None.  A class outside ``classes`` contributes through the softmax only.  The gradient flows into ``logits`` only.  The
    softmax and the products run in double and every output is rounded once; bitwise reproducible."""
    classes = check_boundary_classes(classes)
    labels, classes = _logits_labels("boundary_loss", logits, labels, optional=True, classes=classes)
    B, Cc, H, W = logits.shape
    K = len(classes)
    if not torch.is_tensor(phi) or phi.dtype != torch.float32 or phi.device != logits.device or \
            tuple(phi.shape) not in (((B, H, W), (B, 1, H, W)) if K == 1 else ((B, K, H, W),)):
        raise WsdlError(f"boundary_loss: phi must be a float32 {(B, K, H, W)} tensor on {logits.device}"
                        + (f" (or {(B, H, W)})" if K == 1 else ""))
    phi = phi.detach()
    phi = phi if phi.is_contiguous() else phi.contiguous()
    scale = _device_scalar("boundary_loss", scale, logits.device)
    return _BoundaryLoss.apply(logits, phi, labels, classes, int(ignore_index), scale)


# ---- overlap and focal losses (csrc/overlap_loss.hip; include/wsdl_hip.h "overlap and focal losses") ------------------------
def _finite_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float("inf")


def check_tversky_options(alpha, beta, gamma, smooth, name="tversky_loss"):
    """ValueError unless ``alpha``, ``beta``, ``smooth`` are finite numbers >= 0 and ``gamma`` a finite number > 0 (no device
    needed)."""
    for v, what in ((alpha, "alpha"), (beta, "beta"), (smooth, "smooth")):
        if not _finite_number(v) or v < 0:
            raise ValueError(f"{name}: {what} {v!r} must be a finite number >= 0")
    if not _finite_number(gamma) or gamma <= 0:
        raise ValueError(f"{name}: gamma {gamma!r} must be a finite number > 0")


def check_focal_options(gamma, reduction, name="focal_loss"):
    """ValueError unless ``gamma`` is a finite number >= 0 and ``reduction`` 'mean', 'sum' or 'none' (no device needed)."""
    if not _finite_number(gamma) or gamma < 0:
        raise ValueError(f"{name}: gamma {gamma!r} must be a finite number >= 0")
    if reduction not in _CE_REDUCTIONS:
        raise ValueError(f"{name}: reduction {reduction!r}: 'mean', 'sum' or 'none'")


def check_overlap_classes(classes, C=None, name="tversky_loss"):
    """``classes`` as a tuple of ints: None means all ``C`` classes; otherwise the rules of ``check_boundary_classes`` and,
    with ``C``, every class below it.  ValueError otherwise (no device needed)."""
    if classes is None:
        if C is None:
            return None
        if not 1 <= int(C) <= MAX_BOUNDARY_CLASSES:
            raise ValueError(f"{name}: classes=None lists all C = {C} classes, supported up to {MAX_BOUNDARY_CLASSES}; pass a list")
        return tuple(range(int(C)))
    classes = check_boundary_classes(classes, name)
    if C is not None and max(classes) >= C:
        raise ValueError(f"{name}: classes {classes!r} must be below C = {C}")
    return classes


def overlap_sums(logits, labels, *, classes=None, ignore_index=-100, per_image=False, out=None):
    """float64 (segments, K, 3) on the device - segments = B with ``per_image``, else 1: for the listed class ``c`` and
    ``s = softmax(logits)``, ``[..., 0] = I = sum s_c y_c``, ``[..., 1] = P = sum over valid pixels of s_c`` and ``[..., 2] =
    Y = sum y_c`` (exact), with ``y_c = 1`` where ``labels == c`` and the pixel is valid (``labels != ignore_index``) - what
    soft Dice, Tversky and their relatives are made of (wsdl_overlap_sums: two launches, double accumulation in fixed order,
    bitwise reproducible, no host read).  ``classes``: None for all C, or up to 32 distinct ints.  ``out``: a dict whose
    ``"sums"`` tensor is reused."""
    labels, classes = _logits_labels("overlap_sums", logits, labels, classes=classes)
    logits = _dense(logits.detach(), "logits")
    B, Cc, H, W = logits.shape
    K, S = len(classes), B if per_image else 1
    sums = _out_tensor(out, "sums", (S, K, 3), torch.float64, logits.device)
    ws = workspace(_ws_bytes("wsdl_overlap_workspace", S, K), logits.device)
    cls = (C.c_int * K)(*classes)
    check(lib().wsdl_overlap_sums(_p(logits), _p(labels), cls, K, _p(sums), B, Cc, H, W, int(bool(per_image)), int(ignore_index),
                                  _p(ws), ws.numel(), _stream()))
    return sums


class _TverskyLoss(torch.autograd.Function):
    """wsdl_tversky_fwd_bwd: the loss and its COMPLETE gradient in three launches; the backward multiplies by the upstream
    gradient only."""

    @staticmethod
    def forward(ctx, logits, labels, classes, alpha, beta, gamma, smooth, per_image, present_only, ignore_index, scale):
        logits = _dense(logits, "logits")
        B, Cc, H, W = logits.shape
        K, S = len(classes), B if per_image else 1
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits) if logits.requires_grad else None
        ws = workspace(_ws_bytes("wsdl_overlap_workspace", S, K), logits.device)
        cls = (C.c_int * K)(*classes)
        check(lib().wsdl_tversky_fwd_bwd(_p(logits), _p(labels), cls, K, _p(loss), _p(dl), None, _p(scale), alpha, beta, gamma,
                                         smooth, int(per_image), int(present_only), B, Cc, H, W, int(ignore_index), _p(ws),
                                         ws.numel(), _stream()))
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (_scaled_grad(dl, g),) + (None,) * 10


def tversky_loss(logits, labels, *, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes=None, per_image=False,
                 present_only=False, ignore_index=-100, scale=None):
    """The Tversky loss (Salehi et al., MLMI 2017) on (B,C,H,W) logits and int64 (B,H,W) labels, a 0-dim float32 tensor with
    its gradient (wsdl_tversky_fwd_bwd).  With the sums of ``overlap_sums`` per segment and listed class, ``N = I + smooth`` and
    ``D = I + alpha (P - I) + beta (Y - I) + smooth``: ``T = N / D`` (1 where ``D == 0``), the term is ``(1 - T) ** gamma``
    (exactly 0 with a zero gradient where ``1 - T <= 0``), and the loss is ``scale`` x the mean of the terms over segments and
    classes; ``present_only`` leaves out the classes without a pixel in their segment (``Y == 0``); without a term the loss is
    0.  ``alpha`` weighs false positives and ``beta`` false negatives; ``alpha = beta = 0.5`` is soft Dice (``dice_loss``),
    ``alpha = beta = 1`` the soft Jaccard index.  The focal Tversky loss of Abraham & Khan (ISBI 2019), ``(1 - T) ** (1 /
    gamma_paper)``, is ``gamma = 1 / gamma_paper`` (their 4/3: ``gamma=0.75``).

    ``classes``: None for all C classes, or up to 32 distinct ints; a valid pixel of a class that is not listed is
    background for every listed class.  Pixels with ``labels == ignore_index`` count nowhere and get a gradient of exactly
    0; a batch without a valid pixel gives 0, not NaN.  ``scale``: a one-element float32 device tensor (a weight that changes
    without a new launch plan) or None.  The gradient flows into ``logits`` only.  Everything runs in double and is rounded
    once; three launches, bitwise reproducible, no host read."""
    check_tversky_options(alpha, beta, gamma, smooth)
    labels, classes = _logits_labels("tversky_loss", logits, labels, classes=classes)
    scale = _device_scalar("tversky_loss", scale, logits.device)
    return _TverskyLoss.apply(logits, labels, classes, float(alpha), float(beta), float(gamma), float(smooth), bool(per_image),
                              bool(present_only), int(ignore_index), scale)


def dice_loss(logits, labels, *, smooth=1.0, classes=None, per_image=False, present_only=False, ignore_index=-100, scale=None):
    """The soft Dice loss ``1 - (2 I + smooth) / (P + Y + smooth)``, averaged over segments and classes: it IS
    ``tversky_loss(alpha=0.5, beta=0.5, gamma=1, smooth=smooth / 2)`` - with ``alpha = beta = 1/2`` the Tversky index is
    ``(I + smooth / 2) / ((P + Y) / 2 + smooth / 2)``, the same number - bit for bit, and takes its other options."""
    check_tversky_options(0.5, 0.5, 1.0, smooth, "dice_loss")
    return tversky_loss(logits, labels, alpha=0.5, beta=0.5, gamma=1.0, smooth=smooth / 2.0, classes=classes,
                        per_image=per_image, present_only=present_only, ignore_index=ignore_index, scale=scale)


class _FocalLoss(torch.autograd.Function):
    """wsdl_focal_fwd_bwd: the loss and its un-normalised gradient in one kernel; the backward as in ``_SoftmaxCEEx``."""

    @staticmethod
    def forward(ctx, logits, labels, gamma, ignore_index, weight, pixel_weight, reduction):
        logits = _dense(logits, "logits")
        B, Cc, H, W = logits.shape
        none = reduction == 2
        loss = torch.empty((B, H, W) if none else (), device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits) if logits.requires_grad else None
        inv = None if none else torch.empty(1, device=logits.device, dtype=torch.float32)
        ws = workspace(lib().wsdl_reduce_workspace(), logits.device)
        check(lib().wsdl_focal_fwd_bwd(_p(logits), _p(labels), _p(loss), _p(dl), _p(inv), B, Cc, H, W, gamma, int(ignore_index),
                                       _p(weight), _p(pixel_weight), int(reduction), _p(ws), ws.numel(), _stream()))
        ctx.none = none
        ctx.save_for_backward(dl, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, inv = ctx.saved_tensors
        if not ctx.none:
            return (_scaled_grad(dl, g, inv),) + (None,) * 6       # upstream gradient x 1 / denominator
        out = torch.empty_like(dl)
        B, Cc, H, W = dl.shape
        check(lib().wsdl_scale_by_pixel(_p(dl), _p(_dense(g, "upstream gradient")), _p(out), B, Cc, H, W, _stream()))
        return out, None, None, None, None, None, None


def focal_loss(logits, labels, *, gamma=2.0, weight=None, ignore_index=-100, reduction="mean", pixel_weight=None):
    """The focal loss of Lin et al. (ICCV 2017) in its softmax form on (B,C,H,W) logits and int64 (B,H,W) labels: per pixel
    ``pixel_weight * weight[y] * (1 - s_y) ** gamma * (-log s_y)`` with ``s = softmax(logits)``, forward and gradient in one
    kernel (wsdl_focal_fwd_bwd).  The options are those of ``cross_entropy`` without smoothing: ``weight`` (C,) float32
    (the paper's alpha_t), ``pixel_weight`` (B,H,W) float32 >= 0 (0 = ignore the pixel), ``reduction`` 'mean' | 'sum' |
    'none'; 'mean' divides by the sum of ``pixel_weight * weight[label]`` over the pixels that are not ignored, so ``gamma=0``
    is the weighted cross entropy (0 / 0 gives NaN).  A label outside [0, C) other than ``ignore_index`` gives NaN.
    ``gamma`` >= 0.  ``1 - s_y`` is formed as the sum of the other classes' probabilities and the result is finite for every
    finite logit; everything runs in double and is rounded once.  The gradient flows into ``logits`` only."""
    check_focal_options(gamma, reduction)
    labels, _ = _logits_labels("focal_loss", logits, labels)
    B, Cc, H, W = logits.shape
    for t, name, shape in ((weight, "weight", (Cc,)), (pixel_weight, "pixel_weight", (B, H, W))):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise WsdlError(f"focal_loss: {name} must be a float32 tensor")
        if tuple(t.shape) != shape:
            raise WsdlError(f"focal_loss: {name} {tuple(t.shape)} must be {shape}")
        if t.device != logits.device:
            raise WsdlError(f"focal_loss: {name} is on {t.device}, the logits on {logits.device}")
    weight = None if weight is None else weight.detach().contiguous()
    pixel_weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    return _FocalLoss.apply(logits, labels, float(gamma), int(ignore_index), weight, pixel_weight, _CE_REDUCTIONS[reduction])


def check_percentile(percentile):
    """ValueError unless ``percentile`` is a number in (0, 100] (no device needed)."""
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)) or not 0.0 < percentile <= 100.0:
        raise ValueError(f"surface distances: percentile {percentile!r} must be a number in (0, 100]")
    return float(percentile)


SURFACE_MAX_DIAG2 = 1 << 24             # H^2 + W^2 below this: every squared distance is an exact float32


def surface_distance_stats(preds, labels, value=1, *, percentile=95.0, out=None):
    """The per-image statistics of the surface distances between ``preds == value`` and ``labels == value`` (int64, bool or
    uint8 device maps (B,H,W)), as a dict of device tensors - no host read; ``surface_distances_from_stats`` turns a host copy
    into the Hausdorff distance, its percentile and the average symmetric surface distance.

    The surface ``S(M)`` of a mask is its pixels with a 4-neighbour outside the mask or outside the image (``d2_out == 1``
    of ``edt(M, value, border=True)``; ``M ^ binary_erosion(M)`` with ``border_value=0``, medpy's surface).  The directed set
    A -> B is ``{ D_B[p] : p in S(A) }`` with ``D_B`` the Euclidean distance to the nearest pixel of ``S(B)``.  Index 0 of the
    last axis is pred -> gt, index 1 is gt -> pred:

    ``n`` int64 (B,2) the surface pixel counts; ``max_d2`` int32 (B,2) the largest squared distance, exact; ``sum_d`` float64
    (B,2) the sum of ``sqrt(d2)`` (partials and a fixed-order finalize: bitwise reproducible); ``pct_d2`` float32 (B,2) the
    NEAREST-RANK ``percentile`` of ``d2`` - the ``min(n, 1 + floor((1 - percentile / 100) n))``-th largest, by ``kth_value``.
    Where the other surface is empty every distance is ``EDT_FAR``; where the own surface is empty ``n = 0``, ``max_d2 = 0``,
    ``sum_d = 0`` and ``pct_d2 = +inf`` (``kth_value``'s empty run).  ``H^2 + W^2 < 2^24`` so that ``float(d2)`` is exact.
    ``out``: a dict whose tensors (the four results and the intermediates) are reused.  The last step, the (2,B) -> (B,2) copy of
    the percentiles, is a kernel of the tensor library: the call serves evaluation, a launch plan would not see that copy."""
    percentile = check_percentile(percentile)
    value = _int_option(value, "surface_distance_stats: value")
    preds, labels = _edt_labels(preds, "surface_distance_stats"), _edt_labels(labels, "surface_distance_stats")
    if preds.shape != labels.shape or preds.device != labels.device:
        raise WsdlError(f"surface_distance_stats: preds {tuple(preds.shape)} on {preds.device} / labels {tuple(labels.shape)} on "
                        f"{labels.device} must match")
    B, H, W = labels.shape
    if H * H + W * W >= SURFACE_MAX_DIAG2:
        raise WsdlError(f"surface_distance_stats: H^2 + W^2 = {H * H + W * W} must be below 2^24 (float(d2) must be exact)")
    dev = labels.device
    bufs = out if out is not None else {}

    def buf(key, shape, dtype):
        return _out_tensor(bufs, key, shape, dtype, dev)

    da, _ = edt(preds, value, border=True, want=("out",), out={"out": buf("d2_pred", (B, H, W), torch.int32)})
    db, _ = edt(labels, value, border=True, want=("out",), out={"out": buf("d2_gt", (B, H, W), torch.int32)})
    sa, sb = buf("surf_pred", (B, H, W), torch.int64), buf("surf_gt", (B, H, W), torch.int64)
    check(lib().wsdl_surface_map(_p(da), _p(db), _p(sa), _p(sb), sa.numel(), _stream()))
    _, to_a = edt(sa, 1, want=("in",), out={"in": buf("to_pred", (B, H, W), torch.int32)})
    _, to_b = edt(sb, 1, want=("in",), out={"in": buf("to_gt", (B, H, W), torch.int32)})
    n = buf("n", (B, 2), torch.int64)
    max_d2 = buf("max_d2", (B, 2), torch.int32)
    sum_d = buf("sum_d", (B, 2), torch.float64)
    pct = buf("pct_d2", (B, 2), torch.float32)
    vals, valid = buf("values", (2, B, H, W), torch.float32), buf("valid", (2, B, H, W), torch.uint8)
    ws = workspace(lib().wsdl_surface_stats_workspace(B), dev)
    check(lib().wsdl_surface_stats(_p(da), _p(db), _p(to_a), _p(to_b), B, H, W, _p(n), _p(max_d2), _p(sum_d), _p(vals),
                                   _p(valid), _p(ws), ws.numel(), _stream()))
    kth = buf("pct_rows", (2, B), torch.float32)
    kn = buf("pct_n", (2, B), torch.int64)
    for d in range(2):
        kth_value(vals[d], k=1, frac=1.0 - percentile / 100.0, largest=True, valid=valid[d], segments=B,
                  out={"value": kth[d], "n_valid": kn[d]})
    pct.copy_(kth.t())
    return {"n": n, "max_d2": max_d2, "sum_d": sum_d, "pct_d2": pct}


def surface_distances_from_stats(stats):
    """Host arithmetic on a host copy of ``surface_distance_stats`` (a dict of anything ``np.asarray`` takes, (images, 2)
    each).  Per image: ``hd = sqrt(max(max_d2))``, the Hausdorff distance; ``hd95 = sqrt(max(pct_d2))``, the maximum of the
    two directed percentiles - MONAI's convention, with the nearest-rank percentile instead of its linear interpolation;
    ``assd = (sum_d[0] + sum_d[1]) / (n[0] + n[1])``, the average symmetric surface distance in its POOLED form - medpy
    averages the two directed means instead.  An image where either surface is empty gets ``nan`` for all three and is left
    out of the means.  Returns ``(per_image, means, n_defined)``: a list of dicts, a dict (``nan`` when no image is
    defined) and the number of images the means are taken over."""
    n = np.asarray(stats["n"]).reshape(-1, 2)
    max_d2 = np.asarray(stats["max_d2"]).reshape(-1, 2).astype(np.float64)
    sum_d = np.asarray(stats["sum_d"]).reshape(-1, 2).astype(np.float64)
    pct = np.asarray(stats["pct_d2"]).reshape(-1, 2).astype(np.float64)
    if not (len(n) == len(max_d2) == len(sum_d) == len(pct)) or len(n) == 0:
        raise ValueError("surface_distances_from_stats: the four entries must hold the same, non-zero number of images")
    nan = float("nan")
    per = []
    for i in range(len(n)):
        if n[i, 0] == 0 or n[i, 1] == 0:
            per.append({"hd": nan, "hd95": nan, "assd": nan})
        else:
            per.append({"hd": float(np.sqrt(max_d2[i].max())), "hd95": float(np.sqrt(pct[i].max())),
                        "assd": float((sum_d[i, 0] + sum_d[i, 1]) / float(n[i, 0] + n[i, 1]))})
    defined = [p for p in per if p["hd"] == p["hd"]]
    means = {}
    for key in ("hd", "hd95", "assd"):
        acc = 0.0
        for p in defined:
            acc += p[key]
        means[key] = acc / len(defined) if defined else nan
    return per, means, len(defined)


def surface_distances(preds, labels, value=1, *, percentile=95.0):
    """``surface_distances_from_stats`` of ``surface_distance_stats(preds, labels, value, percentile=)``: Hausdorff distance,
    its nearest-rank percentile and the pooled average symmetric surface distance, per image and as means - one host read."""
    rows = surface_stats_rows(surface_distance_stats(preds, labels, value, percentile=percentile))
    return surface_distances_from_stats(surface_stats_from_rows(rows.cpu().numpy()))


def surface_stats_rows(stats, out=None):
    """The four entries of ``surface_distance_stats`` as one float64 (B,8) device tensor - [n, max_d2, sum_d, pct_d2], two
    columns each, every value exact in a double - so that one copy brings them to the host.  ``out``: a float64 (B,8) tensor
    (e.g. rows of a preallocated table) to fill."""
    row = torch.cat([stats[k].to(torch.float64) for k in ("n", "max_d2", "sum_d", "pct_d2")], dim=1)
    if out is None:
        return row
    out.copy_(row)
    return out


def surface_stats_from_rows(rows):
    """The inverse of ``surface_stats_rows`` on a host copy (images, 8): the dict ``surface_distances_from_stats`` takes."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    return {"n": rows[:, 0:2].astype(np.int64), "max_d2": rows[:, 2:4].astype(np.int64), "sum_d": rows[:, 4:6],
            "pct_d2": rows[:, 6:8]}


def pairwise_affinity_loss(preds, image, window=5, sigma_color=0.1, sigma_space=0.0, apply_softmax=True,
                           normalise=0, cache=None):
    """``cache``: ``pairwise_cache(image, window, sigma_color)`` when the image stays fixed over many evaluations."""
    return _PairwiseAffinityLoss.apply(preds, image, window, sigma_color, sigma_space, bool(apply_softmax),
                                       int(normalise), cache)


def pairwise_cache(image, window=5, sigma_color=0.1):
    """The image's colour affinities for the forward half of the window ((window^2-1)/2, B, H, W)."""
    image = _dense(image, "image")
    B, _, H, W = image.shape
    out = torch.empty((window * window - 1) // 2, B, H, W, device=image.device, dtype=torch.float32)
    check(lib().wsdl_pairwise_cache(_p(image), _p(out), B, H, W, int(window), float(sigma_color), _stream()))
    return out


def compute_affinities(image, sigma_color=0.1, sigma_space=5, window_size=5):
    image = _dense(image, "image")
    B, _, H, W = image.shape
    K = window_size * window_size - 1
    out = torch.empty(K, B, 1, H, W, device=image.device, dtype=torch.float32)
    check(lib().wsdl_compute_affinities(_p(image), _p(out), B, H, W, int(window_size), float(sigma_color),
                                        float(sigma_space or 0.0), _stream()))
    return out


def layercam_epilogue(acts, grads, out_hw=(224, 224), alpha=1.0, variant="modular", thresh=None):
    """acts/grads: lists of (B,C,h,w) device tensors -> cam (B,outH,outW) [, uint8 mask]."""
    n = len(acts)
    acts = [_dense(a.detach(), "act") for a in acts]
    grads = [_dense(g.detach(), "grad") for g in grads]
    B = acts[0].shape[0]
    for a, g in zip(acts, grads):
        if a.shape != g.shape or a.shape[0] != B:
            raise WsdlError("layercam: activation / gradient shape mismatch")
    IA = C.c_int * n
    Cs, hs, ws_ = IA(*[a.shape[1] for a in acts]), IA(*[a.shape[2] for a in acts]), IA(*[a.shape[3] for a in acts])
    PA = _vp * n
    pa, pg = PA(*[_p(a) for a in acts]), PA(*[_p(g) for g in grads])
    dev = acts[0].device
    cam = torch.empty(B, out_hw[0], out_hw[1], device=dev, dtype=torch.float32)
    mask = torch.empty(B, out_hw[0], out_hw[1], device=dev, dtype=torch.uint8) if thresh is not None else None
    nbytes = lib().wsdl_layercam_workspace(n, B, Cs, hs, ws_)
    if nbytes == 0:
        raise WsdlError("layercam: bad layer geometry")
    ws = workspace(nbytes, dev)
    var = {"modular": 0, "notebook": 1}[variant]
    check(lib().wsdl_layercam_epilogue(pa, pg, Cs, hs, ws_, n, B, out_hw[0], out_hw[1], float(alpha), var, _p(cam),
                                       float(thresh) if thresh is not None else -1.0, _p(mask), _p(ws), ws.numel(),
                                       _stream()))
    return (cam, mask) if thresh is not None else cam


def keep_largest_batched(masks):
    """(N,H,W) (or (H,W)) uint8 / bool device masks -> uint8 {0,1}: the largest 8-connected component of each mask, the
    first in raster order on area ties, an empty mask stays empty (reference PsuedoMasks.py:15-21, per image on the host
    there).  No host synchronisation."""
    if masks.dtype == torch.bool:
        masks = masks.to(torch.uint8)
    if masks.dtype != torch.uint8:
        raise WsdlError("keep_largest: masks must be uint8 or bool")
    m = _req(masks, "masks", torch.uint8).contiguous()
    m3 = m.view(-1, m.shape[-2], m.shape[-1])
    out = torch.empty_like(m3)
    if m3.numel() == 0:
        return out.view(m.shape)
    n, h, w = m3.shape
    nbytes = lib().wsdl_keep_largest_workspace(n, h, w)
    if nbytes == 0:
        raise WsdlError("keep_largest: bad mask geometry")
    ws = workspace(nbytes, m.device)
    check(lib().wsdl_keep_largest(_p(m3), _p(out), n, h, w, _p(ws), ws.numel(), _stream()))
    return out.view(m.shape)


SRG_THRESH_BY_VALUE = 32               # WSDL_SRG_THRESH_BY_VALUE: thresholds that travel inside the launch
_SRG_BALANCES = {"fg_bg": 0, "class": 1, "none": 2}


def check_connectivity(connectivity, name="label_components"):
    """ValueError unless ``connectivity`` is the int 4 or 8 (no device needed)."""
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f"{name}: connectivity {connectivity!r}: 4 or 8")
    return int(connectivity)


def check_components_geometry(B, H, W, name="label_components"):
    """ValueError for an empty map or one of more than 2^31 - 1 pixels (what the library refuses; no device needed)."""
    if min(B, H, W) <= 0 or B * H * W > 2 ** 31 - 1:
        raise ValueError(f"{name}: (B,H,W) = {(B, H, W)}: positive sizes with B H W <= 2^31 - 1")


def _error_word(out, ws):
    if out is not None:
        out["error"] = ws[:4].view(torch.int32)


def label_components(labels, *, background=None, connectivity=8, want_area=False, out=None):
    """Connected components of int64 device label maps (B,H,W) (a bool / uint8 mask is converted): two pixels of an image
    belong together if they are connected through pixels of the SAME value, ``connectivity`` 8 or 4.  Returns ``comp``, int32
    (B,H,W): at every pixel the raster index ``y * W + x`` of the first pixel of its component - scipy's label order made
    position-independent - and -1 where ``labels == background`` (None: every value forms components); with
    ``want_area=True`` returns ``(comp, area)``, ``area`` int32 (B,H,W) the pixel count of the pixel's component (0 on
    background).

    Many workgroups per image (wsdl_label_components: tiles in LDS, a lock-free union across the tile seams, a flatten pass):
    three launches, four with areas, integer atomics only, no host read, bitwise reproducible - a launch plan can hold the
    call.  ``ops.keep_largest_batched`` keeps its own one-workgroup-per-mask kernel.  ``out``: a dict whose ``"comp"`` /
    ``"area"`` tensors receive the maps (created there when missing or of another shape); ``out["error"]`` then views the
    library's error word in the scratch buffer (int32: 0 unless a union gave up; valid until the next call that uses scratch)."""
    connectivity = check_connectivity(connectivity)
    if background is not None:
        background = _int_option(background, "label_components: background")
    labels = _edt_labels(labels, "label_components")
    B, H, W = labels.shape
    check_components_geometry(B, H, W)
    comp = _out_tensor(out, "comp", (B, H, W), torch.int32, labels.device)
    area = _out_tensor(out, "area", (B, H, W), torch.int32, labels.device) if want_area else None
    ws = workspace(_ws_bytes("wsdl_label_components_workspace", B, H, W), labels.device)
    check(lib().wsdl_label_components(_p(labels), B, H, W, connectivity, int(background is not None), background or 0, _p(comp),
                                      _p(area), _p(ws), ws.numel(), _stream()))
    _error_word(out, ws)
    return (comp, area) if want_area else comp


def srg_thresholds(thresh, C):
    """``thresh`` of seeded region growing as a list of C floats: a number, a ``(bg, fg)`` pair - ``bg`` for class 0, ``fg`` for
    the rest (the paper: 0.99 / 0.85) - or C numbers.  ValueError otherwise (no device needed)."""
    def num(v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError(f"seeded_region_growing: thresh {thresh!r}: a number, a (bg, fg) pair or {C} numbers, none NaN")
        return float(v)
    if isinstance(thresh, (tuple, list)):
        vals = [num(v) for v in thresh]
        if len(vals) == 2:
            return [vals[0]] + [vals[1]] * (C - 1)
        if len(vals) == C:
            return vals
        raise ValueError(f"seeded_region_growing: thresh {thresh!r}: a number, a (bg, fg) pair or {C} numbers")
    return [num(thresh)] * C


def seeded_region_growing(scores, seeds, thresh, *, present=None, ignore_index=255, out=None):
    """Deep seeded region growing (Huang et al., CVPR 2018; the reference has no such step) on the device.  ``scores``
    (B,C,H,W) float32, usually softmax probabilities - they are only compared; ``seeds`` (B,H,W) int64: a value in [0,C) is a
    seed of that class, anything else is unseeded; ``thresh``: a float32 (C,) DEVICE tensor (read by the kernel: its values may
    change under a launch plan), or a number / a ``(bg, fg)`` pair / C numbers (``srg_thresholds``), which travel by value;
    ``present``: optional (B,C) uint8 / bool device tensor, 0 = a class the image cannot contain.

    A pixel is a candidate of the first class of largest score among the present ones if that score is > the class's
    threshold (float32, strict; a NaN score: no candidate).  The candidate map is labelled (``label_components``'s kernels,
    8-connected, same class) and a component grows iff one of its pixels carries a seed of the component's own class.
    Returns ``(grown, counts)``: ``grown`` int64 (B,H,W) = the seed where there is one (seeds are never overwritten), else the
    class of a grown component, else ``ignore_index``; ``counts`` int64 (B,C), the per-image pixels of each class in
    ``grown``, left on the device.  Six launches and a memset, integer atomics only, no host read, bitwise reproducible; the
    inputs are never written.  ``out``: a dict whose ``"grown"`` / ``"counts"`` tensors are filled (created when missing or of
    another shape); ``out["error"]`` then views the labelling's error word (see ``label_components``)."""
    if not torch.is_tensor(scores) or scores.dim() != 4:
        raise WsdlError("seeded_region_growing: scores must be a (B,C,H,W) tensor")
    B, Cc, H, W = scores.shape
    thresh_dev = thresh_host = None
    if torch.is_tensor(thresh):
        if thresh.dtype != torch.float32 or tuple(thresh.shape) != (Cc,):
            raise WsdlError(f"seeded_region_growing: a thresh tensor must be float32 {(Cc,)}")
    else:
        vals = srg_thresholds(thresh, Cc)
    ignore_index = _int_option(ignore_index, "seeded_region_growing: ignore_index")
    check_components_geometry(B, H, W, "seeded_region_growing")
    scores = _dense(scores.detach(), "seeded_region_growing: scores")
    dev = scores.device
    if not torch.is_tensor(seeds) or tuple(seeds.shape) != (B, H, W) or seeds.device != dev:
        raise WsdlError(f"seeded_region_growing: seeds must be a {(B, H, W)} tensor on {dev}")
    seeds = _req(seeds, "seeded_region_growing: seeds", torch.int64).detach().contiguous()
    if torch.is_tensor(thresh):
        if thresh.device != dev:
            raise WsdlError(f"seeded_region_growing: thresh is on {thresh.device}, the scores on {dev}")
        thresh_dev = thresh.detach().contiguous()
    elif Cc <= SRG_THRESH_BY_VALUE:
        thresh_host = (C.c_float * Cc)(*vals)
    else:
        thresh_dev = torch.tensor(vals, dtype=torch.float32).to(dev)
    if present is not None:
        if not torch.is_tensor(present) or tuple(present.shape) != (B, Cc) or present.device != dev \
                or present.dtype not in (torch.uint8, torch.bool):
            raise WsdlError(f"seeded_region_growing: present must be a uint8 / bool {(B, Cc)} tensor on {dev}")
        present = present.to(torch.uint8).contiguous()
    grown = _out_tensor(out, "grown", (B, H, W), torch.int64, dev)
    counts = _out_tensor(out, "counts", (B, Cc), torch.int64, dev)
    ws = workspace(_ws_bytes("wsdl_seeded_region_growing_workspace", B, Cc, H, W), dev)
    check(lib().wsdl_seeded_region_growing(_p(scores), _p(seeds), thresh_host, _p(thresh_dev), _p(present), B, Cc, H, W, ignore_index,
                                           _p(grown), _p(counts), _p(ws), ws.numel(), _stream()))
    _error_word(out, ws)
    return grown, counts


def check_balance(balance, name="balanced_seed_weights"):
    if balance not in _SRG_BALANCES:
        raise ValueError(f"{name}: balance {balance!r}: 'fg_bg', 'class' or 'none'")
    return balance


def balanced_seed_weights(grown, counts, *, balance="fg_bg", out=None):
    """float32 (B,H,W) pixel weights of the seeding loss from ``seeded_region_growing``'s ``grown`` (int64 (B,H,W)) and ``counts``
    (int64 (B,C)): a pixel whose label is in [0,C) gets ``float(1.0 / double(B * n))`` with ``n`` the number of pixels of its
    group in its image - ``balance="fg_bg"``: class 0 and the classes >= 1 are the two groups (the paper's 1/|S_bg| and
    1/|S_fg|), ``"class"``: every class by itself, ``"none"``: weight 1.  Any other label gets 0, and so does a group without a
    pixel (the paper divides by zero there).  With ``ops.cross_entropy(..., reduction="sum", pixel_weight=)`` this is the
    batch mean of the balanced seeding loss.  One launch, no host read.  ``out``: a dense float32 (B,H,W) device tensor to fill."""
    check_balance(balance)
    if not torch.is_tensor(grown) or grown.dim() != 3:
        raise WsdlError("balanced_seed_weights: grown must be a (B,H,W) tensor")
    grown = _req(grown, "balanced_seed_weights: grown", torch.int64).detach().contiguous()
    B, H, W = grown.shape
    if not torch.is_tensor(counts) or counts.dim() != 2 or counts.shape[0] != B or counts.shape[1] < 1 or counts.device != grown.device:
        raise WsdlError(f"balanced_seed_weights: counts must be a ({B},C) tensor on {grown.device}")
    counts = _req(counts, "balanced_seed_weights: counts", torch.int64).detach().contiguous()
    check_components_geometry(B, H, W, "balanced_seed_weights")
    if out is None:
        out = torch.empty((B, H, W), device=grown.device, dtype=torch.float32)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (B, H, W) and out.device == grown.device
              and out.is_contiguous()):
        raise WsdlError(f"balanced_seed_weights: out must be a dense float32 {(B, H, W)} tensor on {grown.device}")
    check(lib().wsdl_balanced_seed_weights(_p(grown), _p(counts), B, counts.shape[1], H, W, _SRG_BALANCES[balance], _p(out), _stream()))
    return out


SLIC_MAX_STEP, SLIC_MAX_COMPACTNESS, SLIC_MAX_SIDE = 128, 255, 8192
SUPERPIXEL_MAX_CHANNELS, SUPERPIXEL_MAX_CLASSES = 32, 64
_SLIC_MEAN = (0.485, 0.456, 0.406)
_SLIC_STD = (0.229, 0.224, 0.225)
_slic_norm_cache = {}


def check_slic_options(step, compactness=10, num_iter=10, min_size=None, name="slic"):
    """``(step, compactness, num_iter, min_size)`` as ints, ``min_size=None`` resolved to ``max(1, step * step // 4)``;
    ValueError unless step is an int in [1, 128], compactness an int in [1, 255], num_iter an int >= 0 and min_size an int >= 1
    (what the library refuses; no device needed)."""
    def integer(v, what, lo, hi=None):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"{name}: {what} {v!r}: an int " + (f"in [{lo}, {hi}]" if hi is not None else f">= {lo}"))
        return int(v)
    step = integer(step, "step", 1, SLIC_MAX_STEP)
    compactness = integer(compactness, "compactness", 1, SLIC_MAX_COMPACTNESS)
    num_iter = integer(num_iter, "num_iter", 0)
    min_size = max(1, step * step // 4) if min_size is None else integer(min_size, "min_size", 1)
    return step, compactness, num_iter, min_size


def check_slic_geometry(B, H, W, name="slic"):
    """ValueError for an empty batch, a side above 8192 or more than 2^31 - 1 pixels (what the library refuses; no device needed)."""
    check_components_geometry(B, H, W, name)
    if max(H, W) > SLIC_MAX_SIDE:
        raise ValueError(f"{name}: (H,W) = {(H, W)}: sides up to {SLIC_MAX_SIDE}")


def slic_grid(H, W, step):
    """``(GH, GW)`` of the superpixel grid: ``max(1, (H + step // 2) // step)`` and likewise for W."""
    return max(1, (H + step // 2) // step), max(1, (W + step // 2) // step)


def slic_max_segments(H, W, step, min_size=None):
    """The bound ``K + (H * W) // min_size + 1`` on the segments of one image that ``slic`` can return: the K main components and
    pixel 0's, plus every other kept component (each has at least ``min_size`` pixels).  The size every per-segment buffer is
    allocated with.  No device needed."""
    step, _, _, min_size = check_slic_options(step, min_size=min_size, name="slic_max_segments")
    GH, GW = slic_grid(H, W, step)
    return GH * GW + (H * W) // min_size + 1


def slic_launches(H, W, num_iter):
    """Kernel launches of one ``slic`` call: ``8 + L + max(1, 2 * num_iter)`` with L = 4 labelling launches, 3 when the image
    is a single labelling tile (H <= 32 and W <= 64)."""
    return 8 + (3 if H <= 32 and W <= 64 else 4) + max(1, 2 * num_iter)


def slic_quantize(images, mean=_SLIC_MEAN, std=_SLIC_STD):
    """Float device images (B,3,H,W), normalised as ``(x - mean) / std`` per channel, back to uint8:
    ``clamp(rint((x * std + mean) * 255), 0, 255)`` with plain tensor operations on the device.  Plumbing in front of ``slic``,
    not part of its exact contract."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or not images.is_floating_point():
        raise WsdlError("slic_quantize: images must be a float (B,3,H,W) tensor")
    if not images.is_cuda:
        raise WsdlError(f"slic_quantize: the HIP path needs a device tensor (got {images.device}); there is no CPU fallback")
    x = images.detach()
    key = (x.device, x.dtype, tuple(mean), tuple(std))
    if key not in _slic_norm_cache:          # made once: a tensor from host values is a copy the host waits for
        _slic_norm_cache[key] = (torch.tensor(key[2], dtype=x.dtype, device=x.device).view(1, 3, 1, 1),
                                 torch.tensor(key[3], dtype=x.dtype, device=x.device).view(1, 3, 1, 1))
    m, s = _slic_norm_cache[key]
    return torch.clamp(torch.round((x * s + m) * 255), 0, 255).to(torch.uint8).contiguous()


def slic(images, step, compactness=10, num_iter=10, min_size=None, out=None):
    """Integer SLIC superpixels (Achanta et al., TPAMI 2012, pixel-centric as in gSLIC; the reference has no such step) of uint8
    device images (B,3,H,W) - the three channels are used as given; float images go through ``slic_quantize`` first.  ``step``
    (S, 1 to 128) is the spacing of the initial grid, ``compactness`` (m, 1 to 255) the weight of position against colour,
    ``num_iter`` the number of assign / update rounds (0: one assignment against the initial centres), ``min_size`` (None:
    ``max(1, S * S // 4)``) the area below which a stray component is merged away.

    All arithmetic is integer, in units of 1/16 (include/wsdl_hip.h "SLIC superpixels" and tests/slic_oracle.py state it in
    full): a pixel takes, among the centres of the 3 x 3 grid cells around its own, the one of smallest
    ``D = S^2 |16 I - c|^2 + m^2 |16 (y, x) - (cy, cx)|^2`` (64 bits; ties to the smallest index), a centre becomes the rounded
    mean ``(16 sum + n // 2) // n`` of its pixels.  The last assignment is labelled 4-connected (``label_components``' kernels,
    with areas); a component that is not the largest of its label, is smaller than ``min_size`` and does not start at pixel 0 is
    merged into the component of the pixel left of its first pixel (above it in column 0) - chains of such merges of any length.
    Returns ``(segments, n_segments)``: ``segments`` int32 (B,H,W), dense ids in ``[0, n_b)`` ordered by each segment's first
    pixel, every segment 4-connected; ``n_segments`` int32 (B,) on the device, at most ``slic_max_segments(H, W, step, min_size)``.

    ``slic_launches(H, W, num_iter)`` = ``8 + L + max(1, 2 * num_iter)`` launches (L = 4, or 3 for an image of one 64 x 32
    labelling tile), integer atomics only, no float anywhere, no host read, parameters by value, bitwise reproducible - a launch
    plan can hold the call; the images are never written.  ``out``: a dict whose ``"segments"`` / ``"n_segments"`` / ``"raw"``
    (int32 (B,H,W): the last assignment) / ``"centres"`` (int32 (B,K,5): y, x, c0, c1, c2 times 16) tensors are filled (created
    when missing or of another shape); ``out["error"]`` then views the labelling's error word (see ``label_components``)."""
    step, compactness, num_iter, min_size = check_slic_options(step, compactness, num_iter, min_size)
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
        raise WsdlError("slic: images must be a (B,3,H,W) uint8 tensor")
    if images.dtype != torch.uint8:
        raise ValueError(f"slic: images must be uint8, got {images.dtype} (float images: slic_quantize)")
    B, _, H, W = images.shape
    check_slic_geometry(B, H, W)
    images = _req(images, "slic: images", torch.uint8).contiguous()
    dev = images.device
    GH, GW = slic_grid(H, W, step)
    segments = _out_tensor(out, "segments", (B, H, W), torch.int32, dev)
    n_segments = _out_tensor(out, "n_segments", (B,), torch.int32, dev)
    keep = out if out is not None else {}
    raw = _out_tensor(keep, "raw", (B, H, W), torch.int32, dev)
    centres = _out_tensor(keep, "centres", (B, GH * GW, 5), torch.int32, dev)
    ws = workspace(_ws_bytes("wsdl_slic_workspace", B, H, W, step), dev)
    check(lib().wsdl_slic(_p(images), B, H, W, step, compactness, num_iter, min_size, _p(raw), _p(centres), _p(segments),
                          _p(n_segments), _p(ws), ws.numel(), _stream()))
    _error_word(out, ws)
    return segments, n_segments


def _superpixel_segments(segments, shape, dev, name):
    if not torch.is_tensor(segments) or tuple(segments.shape) != tuple(shape) or segments.device != dev:
        raise WsdlError(f"{name}: segments must be an int32 {tuple(shape)} tensor on {dev}")
    return _req(segments, f"{name}: segments", torch.int32).contiguous()


def _segments_max(n, name):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"{name}: n_segments_max {n!r}: an int >= 1 (slic_max_segments)")
    return int(n)


def _superpixel_pool(values, segments, n_segments_max, out, snap, name):
    n_max = _segments_max(n_segments_max, name)
    if not torch.is_tensor(values) or values.dim() != 4:
        raise WsdlError(f"{name}: values must be a (B,C,H,W) float32 tensor")
    B, Cc, H, W = values.shape
    if not 1 <= Cc <= SUPERPIXEL_MAX_CHANNELS:
        raise ValueError(f"{name}: {Cc} channels: 1 to {SUPERPIXEL_MAX_CHANNELS}")
    check_components_geometry(B, H, W, name)
    values = _dense(values.detach(), f"{name}: values")
    dev = values.device
    segments = _superpixel_segments(segments, (B, H, W), dev, name)
    nbytes = _ws_bytes("wsdl_superpixel_workspace", B, Cc, n_max)
    if nbytes == 0:
        raise WsdlError(f"{name}: B C n_segments_max = {B * Cc * n_max} > 2^31 - 1")
    mean = _out_tensor(out, "mean", (B, Cc, n_max), torch.float32, dev)
    count = _out_tensor(out, "count", (B, n_max), torch.int32, dev)
    snapped = _out_tensor(out, "snapped", (B, Cc, H, W), torch.float32, dev) if snap else None
    ws = workspace(nbytes, dev)
    check(lib().wsdl_superpixel_mean(_p(values), _p(segments), B, Cc, H, W, n_max, _p(mean), _p(count), _p(snapped), _p(ws),
                                     ws.numel(), _stream()))
    return mean, count, snapped


def superpixel_mean(values, segments, n_segments_max, out=None):
    """The mean of float32 device ``values`` (B,C,H,W), C up to 32, over every segment of ``segments`` (int32 (B,H,W), as ``slic``
    returns them): ``(mean, count)`` with ``mean`` float32 (B,C,n_segments_max) and ``count`` int32 (B,n_segments_max).  No float
    atomics: every value is quantised to ``q = llrint(double(clamp(v, -2^15, 2^15)) * 2^24)``, the q are summed with 64-bit
    integer atomics (on chip per tile first) and ``mean = float(double(sum) / (double(n) * 2^24))`` - independent of the order,
    bit for bit the oracle's value; within 2^-24 (plus the rounding to float32) of the exact mean of values inside +-2^15.
    0 where ``n = 0``; NaN for an (image, channel, segment) that saw a NaN.  A pixel whose id is outside
    ``[0, n_segments_max)`` is not pooled.  Two launches and two memsets, no host read.  ``out``: a dict whose ``"mean"`` /
    ``"count"`` tensors are filled (created when missing or of another shape)."""
    mean, count, _ = _superpixel_pool(values, segments, n_segments_max, out, False, "superpixel_mean")
    return mean, count


def superpixel_snap(values, segments, n_segments_max, out=None):
    """(B,C,H,W) float32: every pixel gets the ``superpixel_mean`` of its segment (0 at an id outside ``[0, n_segments_max)``) -
    the mean pass plus a gather, three launches.  ``out``: a dict whose ``"snapped"`` (and ``"mean"`` / ``"count"``) tensors are
    filled."""
    return _superpixel_pool(values, segments, n_segments_max, out, True, "superpixel_snap")[2]


def superpixel_vote(labels, segments, n_segments_max, num_classes, ignore_index=255):
    """int64 (B,H,W): every pixel gets the majority label of its segment among the values of ``labels`` (int64 (B,H,W)) in
    ``[0, num_classes)``, the smallest class on ties; ``ignore_index`` for a segment without such a pixel (and at a segment id
    outside ``[0, n_segments_max)``).  Integer counts, ``num_classes`` up to 64; three launches and a memset, no host read."""
    n_max = _segments_max(n_segments_max, "superpixel_vote")
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= num_classes <= SUPERPIXEL_MAX_CLASSES:
        raise ValueError(f"superpixel_vote: num_classes {num_classes!r}: an int in [1, {SUPERPIXEL_MAX_CLASSES}]")
    ignore_index = _int_option(ignore_index, "superpixel_vote: ignore_index")
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise WsdlError("superpixel_vote: labels must be a (B,H,W) int64 tensor")
    B, H, W = labels.shape
    check_components_geometry(B, H, W, "superpixel_vote")
    labels = _req(labels, "superpixel_vote: labels", torch.int64).detach().contiguous()
    dev = labels.device
    segments = _superpixel_segments(segments, (B, H, W), dev, "superpixel_vote")
    if B * n_max * int(num_classes) > 2 ** 31 - 1:
        raise WsdlError(f"superpixel_vote: B n_segments_max num_classes = {B * n_max * int(num_classes)} > 2^31 - 1")
    out = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    ws = workspace(4 * B * n_max * int(num_classes), dev)
    check(lib().wsdl_superpixel_vote(_p(labels), _p(segments), B, H, W, n_max, int(num_classes), ignore_index, _p(out), _p(ws),
                                     ws.numel(), _stream()))
    return out


def plane_relu_minmax(x):
    """(..., h, w) -> per plane: r = relu(x) - min(relu(x)); r / (max(r) + 1e-8)  (the reference's in-place
    ``cam -= cam.min(); cam /= cam.max() + 1e-8``: the maximum is taken AFTER the minimum has been subtracted)."""
    x = _dense(x, "x")
    hw = x.shape[-1] * x.shape[-2]
    y = torch.empty_like(x)
    check(lib().wsdl_plane_relu_minmax(_p(x), _p(y), x.numel() // hw, hw, _stream()))
    return y


def adam_step_flat(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, step_dev=None, hyper_dev=None):
    """``step_dev``: device int32 step number (used instead of ``step`` - hipGraph replay).  ``hyper_dev``: device floats
    (lr, beta1, beta2, eps, grad_scale) used instead of the host values (with ``step_dev``): nothing of the launch changes
    when a schedule changes them."""
    for t in (p, g, m, v):
        _req(t, "adam buffer")
    if hyper_dev is not None and step_dev is not None:
        check(lib().wsdl_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper_dev), _p(step_dev), _stream()))
        return
    check(lib().wsdl_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2),
                               float(eps), int(step), _p(step_dev), float(grad_scale), _stream()))


FLAT_ADAM_L2, FLAT_ADAMW, FLAT_SGD = 0, 1, 2      # WSDL_FLAT_* of the header
FLAT_HYPER, FLAT_STATS = 10, 4                    # floats in hyper_dev / stats_dev
FLAT_DECAY_BLOCK = 64                             # floats per entry of a decay table


def grad_norm_partials():
    """Number of double partials the norm's fixed grid writes (its workgroup count)."""
    return lib().wsdl_grad_norm_partials()


def grad_norm(g, hyper_dev, step_dev, stats_dev, partials=None):
    """Global norm of the flat gradient ``g`` in two stream-ordered launches; writes ``stats_dev`` = (total_norm, clip_coef,
    apply, skipped_steps) from ``hyper_dev``'s grad_scale, max_norm and skip_nonfinite (include/wsdl_hip.h).  No
    synchronisation; returns ``stats_dev``.  ``partials``: float64 scratch of ``grad_norm_partials()`` elements."""
    _req(g, "gradient")
    _req(hyper_dev, "hyper_dev")
    _req(stats_dev, "stats_dev")
    _req(step_dev, "step_dev", torch.int32)
    if hyper_dev.numel() < FLAT_HYPER or stats_dev.numel() < FLAT_STATS or not g.is_contiguous():
        raise WsdlError(f"grad_norm: dense gradient, hyper_dev of {FLAT_HYPER} floats and stats_dev of {FLAT_STATS} floats")
    n_part = grad_norm_partials()
    if partials is None:
        partials = torch.empty(lib().wsdl_grad_norm_workspace() // 8, device=g.device, dtype=torch.float64)
    _req(partials, "partials", torch.float64)
    if partials.numel() < n_part:
        raise WsdlError(f"grad_norm: partials needs {n_part} doubles")
    check(lib().wsdl_grad_sqnorm_partials(_p(g), g.numel(), _p(partials), _stream()))
    check(lib().wsdl_grad_clip_finalize(_p(partials), n_part, _p(hyper_dev), _p(step_dev), _p(stats_dev), _stream()))
    return stats_dev


def flat_step(algo, p, g, m, v, hyper_dev, step_dev, stats_dev=None, decay_blocks=None):
    """One launch of the flat step kernel (``algo``: FLAT_ADAM_L2 | FLAT_ADAMW | FLAT_SGD) over dense buffers; every per-step
    quantity comes from ``hyper_dev`` / ``step_dev`` / ``stats_dev``.  ``decay_blocks``: uint8 per 64 floats (None: decay
    everywhere); ``stats_dev`` None: no clipping, no skip; ``v`` (and for SGD without momentum ``m``) may be None."""
    for t in (p, g, m, v):
        if t is not None:
            _req(t, "optimiser buffer")
            if not t.is_contiguous() or t.numel() != p.numel():
                raise WsdlError("flat_step: buffers must be dense and of one size")
    _req(hyper_dev, "hyper_dev")
    if hyper_dev.numel() < FLAT_HYPER or (stats_dev is not None and _req(stats_dev, "stats_dev").numel() < FLAT_STATS):
        raise WsdlError(f"flat_step: hyper_dev of {FLAT_HYPER} floats, stats_dev of {FLAT_STATS} floats")
    if step_dev is not None:
        _req(step_dev, "step_dev", torch.int32)
    if decay_blocks is not None:
        _req(decay_blocks, "decay_blocks", torch.uint8)
        if decay_blocks.numel() < (p.numel() + FLAT_DECAY_BLOCK - 1) // FLAT_DECAY_BLOCK or not decay_blocks.is_contiguous():
            raise WsdlError("flat_step: decay_blocks needs one dense byte per 64 floats of the buffer")
    check(lib().wsdl_flat_step_dev(int(algo), _p(p), _p(g), _p(m), _p(v), p.numel(), _p(decay_blocks), _p(hyper_dev),
                                   _p(step_dev), _p(stats_dev), _stream()))


# ---- EMA teacher (csrc/ema.hip; include/wsdl_hip.h "EMA teacher") -----------------------------------------------------------
TEACHER_MAX_CLASSES = 64                          # WSDL_TEACHER_MAX_CLASSES
_TEACHER_MODES = {"replace": 0, "ignore": 1}
_EMA_TABLE_MODES = {"ema": 0, "copy": 1}
EMA_ENTRY_DTYPE = np.dtype([("dst", np.uint64), ("src", np.uint64), ("numel", np.int64)])      # wsdl_ema_entry


def _ema_words(name, hyper_ema_dev, step_dev, start_dev, stats_dev):
    _req(hyper_ema_dev, f"{name}: hyper_ema_dev")
    _req(step_dev, f"{name}: step_dev", torch.int32)
    _req(start_dev, f"{name}: start_dev", torch.int32)
    if hyper_ema_dev.numel() < 2 or step_dev.numel() != 1 or start_dev.numel() != 1:
        raise WsdlError(f"{name}: hyper_ema_dev of two floats (decay, warmup), step_dev and start_dev of one int32 each")
    if stats_dev is not None and _req(stats_dev, f"{name}: stats_dev").numel() < FLAT_STATS:
        raise WsdlError(f"{name}: stats_dev of {FLAT_STATS} floats")


def flat_ema(e, p, hyper_ema_dev, step_dev, start_dev, stats_dev=None):
    """In place, one launch: ``e <- float(fma(a, double(p) - double(e), double(e)))`` over dense float32 device buffers of one
    size, ``a = 1 - d``, ``d = decay`` or, with warm-up, ``min(decay, float32((1 + k) / (10 + k)))`` for ``k = step_dev - start_dev - 1``
    updates already applied (``d`` is a float32 either way: with a 53-bit ``9 / (10 + k)`` exact results land on float32 ties,
    which a fused and an unfused multiply-add break differently).  ``hyper_ema_dev``: two device floats (decay, warmup); ``step_dev`` / ``start_dev``: one-element
    int32 device tensors; ``stats_dev``: the flat optimiser's statistics - a skipped step leaves ``e`` untouched (None: no test).
    Decay 0 copies.  A NaN or inf in ``p`` propagates.  No host read, bitwise reproducible.  Returns ``e``."""
    for t, what in ((e, "e"), (p, "p")):
        _req(t, f"flat_ema: {what}")
        if not t.is_contiguous() or t.numel() != e.numel() or t.numel() == 0:
            raise WsdlError("flat_ema: buffers must be dense, of one size and not empty")
    if _shares_memory(e, p):
        raise WsdlError("flat_ema: e shares memory with p")
    _ema_words("flat_ema", hyper_ema_dev, step_dev, start_dev, stats_dev)
    check(lib().wsdl_flat_ema(_p(e), _p(p), e.numel(), _p(hyper_ema_dev), _p(step_dev), _p(start_dev), _p(stats_dev), _stream()))
    return e


def ema_table_entries(pairs, device):
    """The device table of ``ema_table`` for ``pairs`` = [(dst, src)] of dense float32 device tensors of equal size: a uint8
    tensor holding one ``wsdl_ema_entry`` (dst, src, numel) per pair.  The caller keeps the tensors alive and at their
    addresses."""
    rows = np.zeros(len(pairs), dtype=EMA_ENTRY_DTYPE)
    for i, (dst, src) in enumerate(pairs):
        for t, what in ((dst, "dst"), (src, "src")):
            _req(t, f"ema_table: {what}")
            if not t.is_contiguous() or t.numel() == 0:
                raise WsdlError(f"ema_table: {what} of entry {i} must be dense and not empty")
        if dst.numel() != src.numel() or _shares_memory(dst, src):
            raise WsdlError(f"ema_table: entry {i}: dst and src must have one size and share no memory")
        rows[i] = (dst.data_ptr(), src.data_ptr(), dst.numel())
    return torch.from_numpy(rows.view(np.uint8).copy()).to(device)


def ema_table(table_dev, count, hyper_ema_dev, step_dev, start_dev, stats_dev=None, mode="ema"):
    """One launch over the ``count`` tensors of ``table_dev`` (``ema_table_entries``): ``mode`` 'ema' - the update of ``flat_ema``
    on every (dst, src) - or 'copy' - dst = src.  The same skip test as ``flat_ema``.  No host read, bitwise reproducible."""
    if mode not in _EMA_TABLE_MODES:
        raise WsdlError(f"ema_table: mode {mode!r}: 'ema' or 'copy'")
    _req(table_dev, "ema_table: table", torch.uint8)
    if count <= 0 or table_dev.numel() < count * EMA_ENTRY_DTYPE.itemsize or not table_dev.is_contiguous():
        raise WsdlError(f"ema_table: a dense table of {count} entries of {EMA_ENTRY_DTYPE.itemsize} bytes")
    _ema_words("ema_table", hyper_ema_dev, step_dev, start_dev, stats_dev)
    check(lib().wsdl_ema_table(_p(table_dev), int(count), _p(hyper_ema_dev), _p(step_dev), _p(start_dev), _p(stats_dev),
                               _EMA_TABLE_MODES[mode], _stream()))


def check_teacher_targets_options(logits, labels, tau, mode, ignore_index, out, conf, counts, name="teacher_targets"):
    """Host-side validation of ``teacher_targets``, before any device call.  WsdlError for: an unknown ``mode``; a ``tau`` that is
    neither a number (not NaN) nor a one-element float32 tensor; an ``ignore_index`` that is not an int; ``logits`` not a (B,C,H,W)
    float32 tensor with 1 <= C <= 64, ``labels`` not a (B,H,W) int64 tensor of its size, an empty dimension; ``out`` / a ``conf``
    tensor / ``counts`` that is not a dense int64 (B,H,W) / float32 (B,H,W) / int64 (3,) tensor, or that shares memory with an
    input or with another output; tensors that are not on one device."""
    if mode not in _TEACHER_MODES:
        raise WsdlError(f"{name}: mode {mode!r}: 'replace' or 'ignore'")
    if torch.is_tensor(tau):
        if tau.numel() != 1 or tau.dtype != torch.float32:
            raise WsdlError(f"{name}: tau as a tensor must hold one float32")
    elif isinstance(tau, bool) or not isinstance(tau, (int, float)) or tau != tau:
        raise WsdlError(f"{name}: tau {tau!r} must be a number or a one-element float32 device tensor")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise WsdlError(f"{name}: ignore_index {ignore_index!r} must be an int")
    if not isinstance(conf, bool) and not torch.is_tensor(conf):
        raise WsdlError(f"{name}: conf must be True, False or a float32 (B,H,W) tensor to fill")
    tensors = [(logits, "logits", 4, torch.float32), (labels, "labels", 3, torch.int64)]
    for t, what, rank, dtype in tensors:
        if not torch.is_tensor(t) or t.dim() != rank:
            raise WsdlError(f"{name}: {what} must be a tensor of rank {rank}")
        if t.dtype != dtype:
            raise WsdlError(f"{name}: {what} must be {dtype}, got {t.dtype}")
        if t.numel() == 0:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
    B, Cc, H, W = logits.shape
    if Cc > TEACHER_MAX_CLASSES:
        raise WsdlError(f"{name}: logits {tuple(logits.shape)}: at most {TEACHER_MAX_CLASSES} classes")
    if tuple(labels.shape) != (B, H, W):
        raise WsdlError(f"{name}: labels {tuple(labels.shape)} must be {(B, H, W)}, the size of logits {tuple(logits.shape)}")
    outs = []
    for t, what, shape, dtype in ((out, "out", (B, H, W), torch.int64), (conf if torch.is_tensor(conf) else None, "conf", (B, H, W), torch.float32),
                                  (counts, "counts", (3,), torch.int64)):
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and not t.requires_grad):
            raise WsdlError(f"{name}: {what} must be a dense {dtype} {shape} tensor that needs no gradient")
        inputs = [(logits, "logits"), (labels, "labels")] + ([(tau, "tau")] if torch.is_tensor(tau) else [])
        for other, oname in inputs:
            if _shares_memory(t, other):
                raise WsdlError(f"{name}: {what} shares memory with {oname}")
        for o, oname in outs:
            if _shares_memory(t, o):
                raise WsdlError(f"{name}: {what} shares memory with {oname}")
        outs.append((t, what))
        tensors.append((t, what, None, None))
    if torch.is_tensor(tau):
        tensors.append((tau, "tau", None, None))
    device = None                                   # the place last: everything above can be refused without a device
    for t, what, _rank, _dtype in tensors:
        if not t.is_cuda:
            raise WsdlError(f"{name}: {what}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if device is None:
            device = t.device
        elif t.device != device:
            raise WsdlError(f"{name}: {what} is on {t.device}, the other tensors on {device}")


def teacher_targets(logits, labels, tau=0.9, mode="replace", ignore_index=-100, out=None, conf=False, counts=None):
    """Label correction from a teacher's float32 device logits (B,C,H,W), C <= 64, and the current int64 labels (B,H,W), in one
    pass: with ``t`` the first class of largest logit and ``p = float(1 / sum_c exp(double(l_c) - double(l_t)))`` a pixel is
    CONFIDENT iff ``p >= tau`` (a pixel with a non-finite logit never is).  ``mode`` 'replace': a confident pixel with ``t != y``
    takes ``t``; 'ignore': it takes ``ignore_index``; every other pixel - and every pixel that is ``ignore_index`` on input -
    keeps its label.  Returns the corrected labels, or ``(labels, conf)`` with ``conf=True`` (or a float32 (B,H,W) tensor to
    fill): ``p`` at every pixel that is not ignored on input, 0 there and at non-finite pixels.  ``tau``: a number, or a
    one-element float32 device tensor (a schedule changes memory, a launch plan stays).  ``counts``: an int64 (3,) device tensor
    that receives ``+= (kept, changed, ignored on input)`` (exact integer atomics).  ``out``: a dense int64 tensor to fill.  The
    inputs are not modified; no host read; bitwise reproducible."""
    check_teacher_targets_options(logits, labels, tau, mode, ignore_index, out, conf, counts)
    logits = _dense(logits.detach(), "teacher_targets: logits")
    labels = labels.detach().contiguous()
    B, Cc, H, W = logits.shape
    if not torch.is_tensor(tau):
        tau = torch.full((1,), float(tau), device=logits.device, dtype=torch.float32)      # (a fill on the stream: no host read)
    if out is None:
        out = torch.empty_like(labels)
    if conf is True:
        conf = torch.empty(B, H, W, device=logits.device, dtype=torch.float32)
    elif conf is False:
        conf = None
    check(lib().wsdl_teacher_targets(_p(logits), _p(labels), B, Cc, H, W, _p(tau), _TEACHER_MODES[mode], int(ignore_index), _p(out),
                                     _p(conf), _p(counts), _stream()))
    return out if conf is None else (out, conf)


# ---- view consistency: warps of score / label maps, the consistency loss (csrc/consistency.hip) --------------------------------
CONSISTENCY_MAX_CLASSES = 64                        # WSDL_CONSISTENCY_MAX_CLASSES
CONSISTENCY_KINDS = {"kl": 0, "mse": 1, "hard": 2}
CONSISTENCY_TEACHER = {"logits": 0, "probs": 1}
CONSISTENCY_NORMALIZE = {"all": 0, "counted": 1}


def _warp_front(name, src, rows, out_size, fill, rank, dtype):
    """The checks the two warps share -> (out_h, out_w).  ``src``: a device tensor of ``rank`` and ``dtype`` without an empty
    dimension; ``rows``: dense float32 (B,8) on its device."""
    if not torch.is_tensor(src) or src.dim() != rank:
        raise WsdlError(f"{name}: the map must be a tensor of rank {rank}")
    if src.dtype != dtype:
        raise WsdlError(f"{name}: the map must be {dtype}, got {src.dtype}")
    if src.numel() == 0:
        raise WsdlError(f"{name}: the map {tuple(src.shape)} has an empty dimension")
    if rank == 4 and src.shape[1] > CONSISTENCY_MAX_CLASSES:
        raise WsdlError(f"{name}: C = {src.shape[1]}, at most {CONSISTENCY_MAX_CLASSES} channels")
    B = src.shape[0]
    if not torch.is_tensor(rows) or rows.dtype != torch.float32 or tuple(rows.shape) != (B, 8):
        raise WsdlError(f"{name}: rows must be a float32 {(B, 8)} tensor (a00 a01 a02 a10 a11 a12 gain bias per item)")
    if fill not in AUGMENT_FILLS:
        raise WsdlError(f"{name}: fill {fill!r}: 'ignore' or 'reflect'")
    h, w = src.shape[-2:]
    out_h, out_w = (h, w) if out_size is None else (int(v) for v in out_size)
    for a, b, what in ((h, w, "the map"), (out_h, out_w, "out_size")):
        if not (1 <= a <= AUGMENT_MAX_SIDE and 1 <= b <= AUGMENT_MAX_SIDE):
            raise WsdlError(f"{name}: {what} {(a, b)}: side lengths 1..{AUGMENT_MAX_SIDE}")
    if not src.is_cuda:
        raise WsdlError(f"{name}: the HIP path needs a device tensor (got {src.device}); there is no CPU fallback")
    if rows.device != src.device:
        raise WsdlError(f"{name}: rows are on {rows.device}, the map on {src.device}")
    return out_h, out_w


def _warp_out(name, out, shape, dtype, src):
    if out is None:
        return torch.empty(shape, device=src.device, dtype=dtype)
    if not (torch.is_tensor(out) and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()
            and out.device == src.device and not out.requires_grad):
        raise WsdlError(f"{name}: out must be a dense {dtype} {tuple(shape)} tensor on {src.device} that needs no gradient")
    if _shares_memory(out, src):
        raise WsdlError(f"{name}: out shares memory with the input")
    return out


def _warp_scores_fwd(x, rows, out_hw, fill, pad_value, photometric, valid, out):
    B, Cc, h, w = x.shape
    check(lib().wsdl_warp_scores_fwd(_p(x), _p(rows), B, Cc, h, w, out_hw[0], out_hw[1], AUGMENT_FILLS[fill], float(pad_value),
                                     int(bool(photometric)), _p(out), _p(valid), _stream()))


class _WarpScores(torch.autograd.Function):
    """wsdl_warp_scores_fwd and, for the gradient into the source, its adjoint wsdl_warp_scores_bwd."""

    @staticmethod
    def forward(ctx, scores, rows, out_hw, fill, pad_value, photometric, valid, out):
        _warp_scores_fwd(scores.detach().contiguous(), rows, out_hw, fill, pad_value, photometric, valid, out)
        ctx.mark_dirty(out)                     # (an argument filled in place, the caller's or a new one)
        ctx.save_for_backward(rows)
        ctx.geom = (tuple(scores.shape), out_hw, fill, bool(photometric))
        return out

    @staticmethod
    def backward(ctx, dy):
        (rows,) = ctx.saved_tensors
        (B, Cc, h, w), out_hw, fill, photometric = ctx.geom
        if fill != "ignore":
            raise WsdlError("warp_scores: the gradient for fill='reflect' is not built (the adjoint exists for fill='ignore')")
        dy = _dense(dy, "warp_scores: gradient")
        dsrc = torch.empty(B, Cc, h, w, device=dy.device, dtype=torch.float32)
        check(lib().wsdl_warp_scores_bwd(_p(dy), _p(rows), B, Cc, h, w, out_hw[0], out_hw[1], AUGMENT_FILLS[fill], int(photometric),
                                         _p(dsrc), _stream()))
        return (dsrc,) + (None,) * 7


def warp_scores(scores, rows, out_size=None, *, fill="ignore", pad_value=0.0, photometric=False, valid=False, out=None):
    """Warp a float32 (B,C,h,w) map - logits, probabilities, CAMs, images - C <= 64, by the affine rows of an augmentation, in
    one launch (wsdl_warp_scores_fwd).  ``rows`` (B,8) float32 on the device are ``augment.Augment.draw``'s: ``a00 a01 a02 a10
    a11 a12 gain bias``, the map from OUTPUT to source pixel coordinates, applied by exactly the arithmetic of
    ``augment_batch`` (include/wsdl_hip.h), so a prediction is warped as the image it was made from: four clamped taps,
    float32, unfused; ``fill`` "ignore" writes ``pad_value`` where the source point lies outside, "reflect" mirrors the source; a
    non-finite source point is outside under both.  ``photometric=True`` applies ``gain * value + bias`` (the student's IMAGE
    view; leave it off for predictions).  ``out_size`` (out_h, out_w), default the source's.  ``valid=True``: returns ``(out,
    valid)`` with the uint8 (B,out_h,out_w) plane of inside pixels.  ``out``: a dense float32 tensor to fill.

    Differentiable in ``scores`` for ``fill="ignore"``: the backward is the adjoint kernel (wsdl_warp_scores_bwd), a gather in
    double without atomics, bitwise reproducible.  A backward through ``fill="reflect"`` raises.  The input is not modified; no
    host read; results do not depend on B."""
    if not _finite_number(pad_value) and not (isinstance(pad_value, float) and pad_value != pad_value):
        raise WsdlError(f"warp_scores: pad_value {pad_value!r} must be a finite number or NaN")
    out_hw = _warp_front("warp_scores", scores, rows, out_size, fill, 4, torch.float32)
    B, Cc = scores.shape[:2]
    rows = rows.detach().contiguous()
    out = _warp_out("warp_scores", out, (B, Cc) + tuple(out_hw), torch.float32, scores)
    vplane = torch.empty((B,) + tuple(out_hw), device=scores.device, dtype=torch.uint8) if valid else None
    if torch.is_grad_enabled() and scores.requires_grad:
        res = _WarpScores.apply(scores, rows, tuple(out_hw), fill, pad_value, photometric, vplane, out)
    else:
        _warp_scores_fwd(scores.detach().contiguous(), rows, tuple(out_hw), fill, pad_value, photometric, vplane, out)
        res = out
    return (res, vplane) if valid else res


def warp_labels(labels, rows, out_size=None, *, fill="ignore", pad_label=-100, out=None):
    """Warp an int64 (B,h,w) label map by the affine rows of an augmentation (``warp_scores``): the nearest tap
    ``min(floor(xs), w - 1)``, ``pad_label`` where the source point lies outside (the default -100 survives
    ``clamp_max_labels`` and is the cross entropy's default ignore value).  One launch (wsdl_warp_labels); ``out``: a dense int64
    tensor to fill."""
    if isinstance(pad_label, bool) or not isinstance(pad_label, int):
        raise WsdlError(f"warp_labels: pad_label {pad_label!r} must be an int")
    out_hw = _warp_front("warp_labels", labels, rows, out_size, fill, 3, torch.int64)
    B, h, w = labels.shape
    src = labels.detach().contiguous()
    rows = rows.detach().contiguous()
    out = _warp_out("warp_labels", out, (B,) + tuple(out_hw), torch.int64, labels)
    check(lib().wsdl_warp_labels(_p(src), _p(rows), B, h, w, out_hw[0], out_hw[1], AUGMENT_FILLS[fill], int(pad_label), _p(out),
                                 _stream()))
    return out


def _knob_ok(v, lo=None, hi=None, open_lo=False):
    """A host number inside its range (a device float is checked by nobody: it is read by the kernel)."""
    if not _finite_number(v):
        return False
    if lo is not None and (v <= lo if open_lo else v < lo):
        return False
    return hi is None or v <= hi


def check_consistency_options(student_logits, teacher, rows=None, *, kind="kl", teacher_is="logits", temperature=1.0, tau=0.0,
                              lam=1.0, normalize="all", fill="ignore", pixel_weight=None, counts=None, weight_out=None,
                              target_out=None, name="consistency_loss"):
    """Host-side validation of ``consistency_loss``, before any device call; every refusal is a WsdlError naming its cause:
    an unknown ``kind`` / ``teacher_is`` / ``normalize`` / ``fill``; ``temperature`` not a finite number > 0, ``tau`` not a number
    in [0, 1], ``lam`` not a finite number (each may instead be a one-element float32 tensor); ``student_logits`` / ``teacher``
    not float32 tensors of rank 4, an empty dimension, more than 64 classes, different B or C; ``rows`` not a float32 (B,8)
    tensor, or ``rows=None`` with a teacher of another size; ``pixel_weight`` not float32 (B,H,W); ``counts`` / ``weight_out`` /
    ``target_out`` not a dense int64 (2,) / float32 (B,H,W) / int64 (B,H,W) tensor without a gradient, or sharing memory with an
    input or with one another; tensors that are not all on one device - checked last, so everything above is refused without
    a device."""
    for v, table, what in ((kind, CONSISTENCY_KINDS, "kind"), (teacher_is, CONSISTENCY_TEACHER, "teacher_is"),
                           (normalize, CONSISTENCY_NORMALIZE, "normalize"), (fill, AUGMENT_FILLS, "fill")):
        if not isinstance(v, str) or v not in table:
            raise WsdlError(f"{name}: {what} {v!r}: one of {sorted(table)}")
    knobs = []
    for v, what, ok, rule in ((temperature, "temperature", lambda x: _knob_ok(x, 0.0, None, True), "a finite number > 0"),
                              (tau, "tau", lambda x: _knob_ok(x, 0.0, 1.0), "a number in [0, 1]"),
                              (lam, "lam", _knob_ok, "a finite number")):
        if torch.is_tensor(v):
            if v.numel() != 1 or v.dtype != torch.float32:
                raise WsdlError(f"{name}: {what} as a tensor must hold one float32")
            knobs.append((v, what))
        elif not ok(v):
            raise WsdlError(f"{name}: {what} {v!r} must be {rule} or a one-element float32 device tensor")
    tensors = [(student_logits, "student_logits"), (teacher, "teacher")]
    for t, what in tensors:
        if not torch.is_tensor(t) or t.dim() != 4:
            raise WsdlError(f"{name}: {what} must be a (B,C,H,W) tensor")
        if t.dtype != torch.float32:
            raise WsdlError(f"{name}: {what} must be float32, got {t.dtype} (fp16 / bf16 maps are not built)")
        if t.numel() == 0:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
    B, Cc, H, W = student_logits.shape
    if Cc > CONSISTENCY_MAX_CLASSES:
        raise WsdlError(f"{name}: student_logits {tuple(student_logits.shape)}: at most {CONSISTENCY_MAX_CLASSES} classes")
    if tuple(teacher.shape[:2]) != (B, Cc):
        raise WsdlError(f"{name}: teacher {tuple(teacher.shape)} must have B = {B} and C = {Cc} of student_logits {tuple(student_logits.shape)}")
    for a, b, what in ((H, W, "student_logits"), (teacher.shape[2], teacher.shape[3], "teacher")):
        if a > AUGMENT_MAX_SIDE or b > AUGMENT_MAX_SIDE:
            raise WsdlError(f"{name}: {what} {(a, b)}: side lengths 1..{AUGMENT_MAX_SIDE}")
    if rows is None:
        if tuple(teacher.shape) != (B, Cc, H, W):
            raise WsdlError(f"{name}: rows=None reads the teacher directly: its size {tuple(teacher.shape[2:])} must be the "
                            f"student's {(H, W)}; pass rows (augment.relative_rows) to sample it")
    else:
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or tuple(rows.shape) != (B, 8):
            raise WsdlError(f"{name}: rows must be a float32 {(B, 8)} tensor or None")
        tensors.append((rows, "rows"))
    if pixel_weight is not None:
        if not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.float32 or tuple(pixel_weight.shape) != (B, H, W):
            raise WsdlError(f"{name}: pixel_weight must be a float32 {(B, H, W)} tensor or None")
        tensors.append((pixel_weight, "pixel_weight"))
    inputs = list(tensors) + knobs
    outs = []
    for t, what, shape, dtype in ((counts, "counts", (2,), torch.int64), (weight_out, "weight_out", (B, H, W), torch.float32),
                                  (target_out, "target_out", (B, H, W), torch.int64)):
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and not t.requires_grad):
            raise WsdlError(f"{name}: {what} must be a dense {dtype} {shape} tensor that needs no gradient")
        for other, oname in inputs + outs:
            if _shares_memory(t, other):
                raise WsdlError(f"{name}: {what} shares memory with {oname}")
        outs.append((t, what))
    device = None
    for t, what in inputs + outs:
        if not t.is_cuda:
            raise WsdlError(f"{name}: {what}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if device is None:
            device = t.device
        elif t.device != device:
            raise WsdlError(f"{name}: {what} is on {t.device}, the other tensors on {device}")


def _consistency_knobs(tau, lam, temperature, device):
    """The three-float device buffer ``tau lam T`` the kernel reads.  Three one-element views of ONE buffer in this order
    (``wnn.ConsistencyLoss``) are used as they are - no launch, the address stays; anything else is assembled with the tensor
    library's own kernels (which a launch plan does not see: inside a planned step use the module)."""
    vals = (tau, lam, temperature)
    if all(torch.is_tensor(v) for v in vals) and lam.data_ptr() == tau.data_ptr() + 4 and temperature.data_ptr() == tau.data_ptr() + 8 \
            and tau.untyped_storage().data_ptr() == temperature.untyped_storage().data_ptr():
        return tau.detach()
    parts = [v.detach().reshape(1) if torch.is_tensor(v) else torch.full((1,), float(v), device=device, dtype=torch.float32)
             for v in vals]
    return torch.cat(parts)


class _ConsistencyLoss(torch.autograd.Function):
    """wsdl_consistency_fwd_bwd: the loss and its gradient (lam / N included) from one call; the backward multiplies by the
    upstream gradient (``_scaled_grad``)."""

    @staticmethod
    def forward(ctx, z, teacher, rows, pixel_weight, knobs, kind, teacher_is, normalize, fill, counts, weight_out, target_out):
        need = z.requires_grad
        z = _dense(z, "student_logits")
        B, Cc, H, W = z.shape
        loss = torch.empty((), device=z.device, dtype=torch.float32)
        dl = torch.empty_like(z) if need else None
        ws = workspace(lib().wsdl_consistency_workspace(), z.device)
        check(lib().wsdl_consistency_fwd_bwd(_p(z), _p(teacher), _p(rows), _p(pixel_weight), _p(knobs), B, Cc, H, W,
                                             teacher.shape[2], teacher.shape[3], CONSISTENCY_KINDS[kind],
                                             CONSISTENCY_TEACHER[teacher_is], CONSISTENCY_NORMALIZE[normalize], AUGMENT_FILLS[fill],
                                             _p(loss), _p(dl), _p(counts), _p(weight_out), _p(target_out), _p(ws), ws.numel(),
                                             _stream()))
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (_scaled_grad(dl, g),) + (None,) * 11


def consistency_loss(student_logits, teacher, rows=None, *, kind="kl", teacher_is="logits", temperature=1.0, tau=0.0, lam=1.0,
                     normalize="all", fill="ignore", pixel_weight=None, counts=None, weight_out=None, target_out=None):
    """The consistency loss between a student's (B,C,H,W) float32 logits and a teacher's prediction, fused with the teacher's
    warp and with its gradient (wsdl_consistency_fwd_bwd) - a 0-dim float32 tensor.  Mean teacher with a consistency cost,
    FixMatch's confident pseudo-targets and SEAM's equivariant regularisation are this one call.

    ``teacher`` (B,C,h_t,w_t): logits (``teacher_is="logits"``: ``q = softmax(t / temperature)``) or probabilities (``"probs"``:
    ``q = t / sum t``, the temperature is not used).  ``rows`` (B,8): the map from the STUDENT's pixel grid to the teacher's
    (``augment.relative_rows``); the teacher is sampled at every student pixel by ``warp_scores``' rule - bit for bit the value
    ``warp_scores(teacher, rows)`` would hold - read once and never materialised.  ``rows=None``: same size, direct read.

    A pixel is COUNTED iff the warp is inside (``fill``), the teacher's values and the student's logits there are finite, and the
    teacher's confidence ``max q >= tau``; its weight is ``w = counted * pixel_weight`` (float32 (B,H,W), default 1).  ``kind``:
    "kl" ``sum_c q_c (log q_c - log s_c)``; "mse" ``mean_c (s_c - q_c)^2`` on the two softmaxes; "hard" ``-log s_t`` with ``t``
    the first class of largest ``q`` (FixMatch in one pass).  The loss is ``lam / N * sum_p w_p l_p`` with ``N = B H W``
    (``normalize="all"``) or ``sum_p w_p`` ("counted"); with no counted pixel it is 0 with exact zero gradients.

    ``tau``, ``lam`` and ``temperature`` are numbers or one-element float32 device tensors - the kernel reads them from
    device memory, so a schedule changes floats and a launch plan stays (``wnn.ConsistencyLoss``).  ``counts``: an int64 (2,)
    tensor that receives ``(pixels inside, pixels counted)``; ``weight_out`` float32 (B,H,W) receives ``w``; ``target_out`` int64
    (B,H,W) the hard target at counted pixels and -100 elsewhere.  The gradient flows into ``student_logits`` only: the teacher
    is a constant.  Softmaxes, loss and gradient are evaluated in double and rounded once; no atomics, no host read; two
    calls give the same bits."""
    check_consistency_options(student_logits, teacher, rows, kind=kind, teacher_is=teacher_is, temperature=temperature, tau=tau,
                              lam=lam, normalize=normalize, fill=fill, pixel_weight=pixel_weight, counts=counts,
                              weight_out=weight_out, target_out=target_out)
    dense = lambda t: None if t is None else t.detach().contiguous()          # noqa: E731
    knobs = _consistency_knobs(tau, lam, temperature, student_logits.device)
    return _ConsistencyLoss.apply(student_logits, dense(teacher), dense(rows), dense(pixel_weight), knobs, kind, teacher_is,
                                  normalize, fill, counts, weight_out, target_out)


# ---- batch mixing: CutMix / ClassMix / copy-paste (csrc/mix.hip; include/wsdl_hip.h "batch mixing") ----------------------------
MIX_MAX_CLASSES = 64                                # WSDL_MIX_MAX_CLASSES
MIX_MAX_BOXES = 8                                   # WSDL_MIX_MAX_BOXES
MIX_KINDS = {"box": 0, "class": 1, "mask": 2}       # WSDL_MIX_BOX / _CLASS / _MASK
MixResult = collections.namedtuple("MixResult", "images labels pixel_weight scores mask mixed_count")
_MIX_OUT_KEYS = ("images", "labels", "pixel_weight", "scores", "mask", "mixed_count")


class _MixTensor(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("channels", C.c_int), ("elem_bytes", C.c_int)]       # wsdl_mix_tensor


def _mix_tensor(name, t, what, rank, dtype, shape=None):
    if not torch.is_tensor(t) or t.dim() != rank:
        raise WsdlError(f"{name}: {what} must be a tensor of rank {rank}")
    if t.dtype != dtype:
        raise WsdlError(f"{name}: {what} must be {dtype}, got {t.dtype}")
    if t.numel() == 0:
        raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise WsdlError(f"{name}: {what} {tuple(t.shape)} must be {tuple(shape)}")


def _mix_one_device(name, tensors):
    """The place last: everything before can be refused without a device."""
    device = None
    for t, what in tensors:
        if not t.is_cuda:
            raise WsdlError(f"{name}: {what}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if device is None:
            device = t.device
        elif t.device != device:
            raise WsdlError(f"{name}: {what} is on {t.device}, the other tensors on {device}")


def _mix_outs(name, out, keys, specs, inputs):
    """``out``: None or a dict whose entries (of ``keys``) are dense tensors of the wanted shape and type that share no memory
    with an input or with each other -> [(tensor, what)] of the entries given."""
    if out is None:
        return []
    if not isinstance(out, dict) or any(k not in keys for k in out):
        raise WsdlError(f"{name}: out must be a dict with keys from {keys}")
    given = []
    for key, t in out.items():
        if key not in specs:
            raise WsdlError(f"{name}: out[{key!r}] is given but the call does not produce it")
        shape, dtype = specs[key]
        what = f"out[{key!r}]"
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() and not t.requires_grad):
            raise WsdlError(f"{name}: {what} must be a dense {dtype} {tuple(shape)} tensor that needs no gradient")
        for other, oname in inputs + given:
            if _shares_memory(t, other):
                raise WsdlError(f"{name}: {what} shares memory with {oname}")
        given.append((t, what))
    return given


def _mix_candidates(name, candidates, num_classes):
    """The class list as a 64-bit set (None: every class)."""
    if candidates is None:
        return (1 << num_classes) - 1
    word = 0
    try:
        cands = [c for c in candidates]
    except TypeError:
        raise WsdlError(f"{name}: candidates {candidates!r} must be None or a list of classes") from None
    for c in cands:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < num_classes:
            raise WsdlError(f"{name}: candidates {candidates!r}: every entry must be an int in [0, {num_classes})")
        word |= 1 << c
    return word


def check_mix_select_options(class_labels, num_classes, seeds, candidates=None, out=None, name="mix_class_select"):
    """Host-side validation of ``mix_class_select``, before any device call.  WsdlError for: ``num_classes`` not an int in
    [1, 64]; ``class_labels`` not an int64 (B,H,W) tensor, ``seeds`` not an int64 (B,) tensor, an empty dimension, a side over
    16384; ``candidates`` that is neither None nor a list of ints in [0, num_classes); ``out`` that is not a dict of dense int64
    (B,) tensors under 'sel' / 'present', or that shares memory with an input; tensors that are not on one device.  Returns the
    candidates as a 64-bit set."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MIX_MAX_CLASSES:
        raise WsdlError(f"{name}: num_classes {num_classes!r} must be an int in [1, {MIX_MAX_CLASSES}] (the selected set is one 64-bit word)")
    _mix_tensor(name, class_labels, "class_labels", 3, torch.int64)
    B, H, W = class_labels.shape
    if H > AUGMENT_MAX_SIDE or W > AUGMENT_MAX_SIDE:
        raise WsdlError(f"{name}: class_labels {tuple(class_labels.shape)}: side lengths 1..{AUGMENT_MAX_SIDE}")
    _mix_tensor(name, seeds, "seeds", 1, torch.int64, (B,))
    word = _mix_candidates(name, candidates, num_classes)
    inputs = [(class_labels, "class_labels"), (seeds, "seeds")]
    given = _mix_outs(name, out, ("sel", "present"), {"sel": ((B,), torch.int64), "present": ((B,), torch.int64)}, inputs)
    _mix_one_device(name, inputs + given)
    return word


def mix_class_select(class_labels, num_classes, seeds, *, candidates=None, out=None):
    """The ClassMix class choice, on the device: for every item i of the int64 (B,H,W) label map ``class_labels`` the classes that
    are PRESENT and half of them SELECTED, as two int64 (B,) tensors of 64-bit sets -> ``(sel, present)``; ``num_classes`` <= 64.

    ``present_i`` = the candidates c (``candidates``: a list of classes, default all of ``range(num_classes)``) for which some
    pixel has ``class_labels[i] == c`` - a label outside ``[0, num_classes)`` (-100, 255) counts for nothing; n = |present_i|,
    k = ceil(n / 2); ``key(c) = fmix(uint64(seeds[i]) + (c + 1) * 0x9E3779B97F4A7C15)`` modulo 2^64, ``fmix`` the splitmix64
    finaliser; ``sel_i`` = the k present classes with the smallest ``(key, c)``; n = 0 gives the empty set.  With two classes this
    picks background or foreground with equal probability; ``candidates=(1,)`` is copy-paste: the foreground whenever present.
    ``seeds``: an int64 (B,) device tensor (``augment.Mix.draw``), item i uses ``seeds[i]`` for its own label map.

    ``out``: a dict with dense int64 (B,) tensors under 'sel' / 'present' to fill.  ``mix_launches("class", select=True)`` says
    what is issued: a memset of ``present``, the presence launch (one 64-bit integer atomic OR per workgroup) and the selection
    launch.  No host read, bitwise reproducible, the inputs are not modified; a launch plan can hold the call."""
    word = check_mix_select_options(class_labels, num_classes, seeds, candidates, out)
    labels = class_labels.detach().contiguous()
    seeds = seeds.detach().contiguous()
    B, H, W = labels.shape
    out = out or {}
    sel, present = (out.get(k) if out.get(k) is not None else torch.empty(B, dtype=torch.int64, device=labels.device)
                    for k in ("sel", "present"))
    check(lib().wsdl_mix_class_select(_p(labels), _p(seeds), B, int(num_classes), H, W, word, _p(present), _p(sel), _stream()))
    return sel, present


def check_mix_options(images, labels, partner, *, kind, boxes=None, class_labels=None, sel=None, mask=None, invert=False,
                      pixel_weight=None, scores=None, want_mask=False, want_count=False, out=None, name="mix_batch"):
    """Host-side validation of ``mix_batch``, before any device call.  WsdlError - naming the argument - for: an unknown ``kind``;
    ``images`` not a float32 (B,Ci,H,W) tensor, ``labels`` not int64 (B,H,W), ``pixel_weight`` not float32 (B,H,W), ``scores`` not
    float32 (B,Cs,H,W) with Cs <= 64, ``partner`` not int32 (B,); a side over 16384, an empty dimension; ``kind="box"`` without
    ``boxes`` or with boxes that are not int32 (B,R,4), 1 <= R <= 8; ``kind="class"`` without ``class_labels`` (int64 (B,H,W)) or
    without ``sel`` (int64 (B,)); ``kind="mask"`` without ``mask`` (uint8 (B,H,W)); a source argument of another kind; ``invert``,
    ``want_mask``, ``want_count`` that are not bools; ``out`` that is not a dict of dense tensors of the results' shapes and types,
    that names a result the call does not produce, or whose entry shares memory with an input or with another entry (item b
    reads item ``partner[b]``: in-place use is a race); tensors that are not on one device."""
    if kind not in MIX_KINDS:
        raise WsdlError(f"{name}: kind {kind!r}: 'box', 'class' or 'mask'")
    for v, what in ((invert, "invert"), (want_mask, "want_mask"), (want_count, "want_count")):
        if not isinstance(v, bool):
            raise WsdlError(f"{name}: {what} {v!r} must be True or False")
    _mix_tensor(name, images, "images", 4, torch.float32)
    B, _, H, W = images.shape
    if H > AUGMENT_MAX_SIDE or W > AUGMENT_MAX_SIDE:
        raise WsdlError(f"{name}: images {tuple(images.shape)}: side lengths 1..{AUGMENT_MAX_SIDE}")
    _mix_tensor(name, labels, "labels", 3, torch.int64, (B, H, W))
    _mix_tensor(name, partner, "partner", 1, torch.int32, (B,))
    inputs = [(images, "images"), (labels, "labels"), (partner, "partner")]
    specs = {"images": (tuple(images.shape), torch.float32), "labels": ((B, H, W), torch.int64)}
    if pixel_weight is not None:
        _mix_tensor(name, pixel_weight, "pixel_weight", 3, torch.float32, (B, H, W))
        inputs.append((pixel_weight, "pixel_weight"))
        specs["pixel_weight"] = ((B, H, W), torch.float32)
    if scores is not None:
        _mix_tensor(name, scores, "scores", 4, torch.float32)
        if scores.shape[1] > MIX_MAX_CLASSES:
            raise WsdlError(f"{name}: scores {tuple(scores.shape)}: C = {scores.shape[1]}, at most {MIX_MAX_CLASSES} channels")
        if (scores.shape[0],) + tuple(scores.shape[2:]) != (B, H, W):
            raise WsdlError(f"{name}: scores {tuple(scores.shape)} must be (B,Cs,H,W) of the images' {(B, H, W)}")
        inputs.append((scores, "scores"))
        specs["scores"] = (tuple(scores.shape), torch.float32)
    sources = {"box": (("boxes", boxes),), "class": (("class_labels", class_labels), ("sel", sel)), "mask": (("mask", mask),)}
    for k, args in sources.items():
        for what, t in args:
            if k == kind and t is None:
                raise WsdlError(f"{name}: kind={kind!r} needs {what}" + (" (ops.mix_class_select)" if what == "sel" else ""))
            if k != kind and t is not None:
                raise WsdlError(f"{name}: {what} belongs to kind={k!r}, not to kind={kind!r}")
    if kind == "box":
        _mix_tensor(name, boxes, "boxes", 3, torch.int32)
        if boxes.shape[0] != B or boxes.shape[2] != 4:
            raise WsdlError(f"{name}: boxes {tuple(boxes.shape)} must be (B,R,4) with B = {B}: rows (y0, x0, y1, x1)")
        if boxes.shape[1] > MIX_MAX_BOXES:
            raise WsdlError(f"{name}: boxes {tuple(boxes.shape)}: R = {boxes.shape[1]}, at most {MIX_MAX_BOXES} boxes per item")
        inputs.append((boxes, "boxes"))
    elif kind == "class":
        _mix_tensor(name, class_labels, "class_labels", 3, torch.int64, (B, H, W))
        _mix_tensor(name, sel, "sel", 1, torch.int64, (B,))
        inputs += [(class_labels, "class_labels"), (sel, "sel")]
    else:
        _mix_tensor(name, mask, "mask", 3, torch.uint8, (B, H, W))
        inputs.append((mask, "mask"))
    if want_mask:
        specs["mask"] = ((B, H, W), torch.uint8)
    if want_count:
        specs["mixed_count"] = ((B,), torch.int64)
    given = _mix_outs(name, out, _MIX_OUT_KEYS, specs, inputs)
    _mix_one_device(name, inputs + given)


def mix_launches(kind, *, select=False, want_count=False):
    """What one ``mix_batch`` call of ``kind`` issues, as ``{"kernels": n, "memsets": m}`` (the keys of a launch plan's
    ``stats``): ONE kernel, plus a memset of the counts with ``want_count``.  ``select=True`` (``kind="class"`` only) adds the
    ``mix_class_select`` call in front of it: a memset of ``present``, the presence launch and the selection launch."""
    if kind not in MIX_KINDS:
        raise WsdlError(f"mix_launches: kind {kind!r}: 'box', 'class' or 'mask'")
    if select and kind != "class":
        raise WsdlError(f"mix_launches: select=True belongs to kind='class', not to kind={kind!r}")
    return {"kernels": 1 + (2 if select else 0), "memsets": (1 if want_count else 0) + (1 if select else 0)}


def mix_batch(images, labels, partner, *, kind, boxes=None, class_labels=None, sel=None, mask=None, invert=False, pixel_weight=None,
              scores=None, want_mask=False, want_count=False, out=None):
    """CutMix / ClassMix / copy-paste as ONE launch (wsdl_mix_apply): every tensor handed in is mixed by the same binary mask,
    ``out_T[b,...,y,x] = M[b,y,x] ? T[partner[b],...,y,x] : T[b,...,y,x]``.  Returns a ``MixResult`` named tuple ``(images, labels,
    pixel_weight, scores, mask, mixed_count)``, None where nothing was asked for.

    Tensors (all on one device): ``images`` float32 (B,Ci,H,W); ``labels`` int64 (B,H,W); optional ``pixel_weight`` float32
    (B,H,W); optional ``scores`` float32 (B,Cs,H,W), Cs <= 64 (a teacher's logits: the mixed-teacher target).
    ``partner`` int32 (B,): item b is mixed with item ``partner[b]``; a value outside ``[0, B)`` (``augment.Mix`` draws -1) leaves
    item b unmixed - its mask is 0 everywhere; the kernel tests the value before it indexes anything.  Self-partners and
    duplicates are legal.

    The mask ``M[b,y,x]`` in {0,1}, 1 = "take the partner's pixel", by ``kind``:
      "box"    ``boxes`` int32 (B,R,4), 1 <= R <= 8, rows ``(y0, x0, y1, x1)`` half-open in pixels: M = 1 inside the union of the R
               boxes; a box with ``y1 <= y0`` or ``x1 <= x0`` contributes nothing; coordinates outside the image clip implicitly,
               negative ones included.
      "class"  M = 1 iff ``class_labels[partner[b],y,x]`` (int64 (B,H,W)) is a class of the partner's selected set
               ``sel[partner[b]]`` (int64 (B,) of 64-bit sets: ``mix_class_select``); a label outside ``[0, C)`` is never selected.
      "mask"   ``mask`` uint8 (B,H,W): M = ``mask[b] != 0`` (PAMR labels, superpixel-snapped masks ... drive the mix).
    ``invert=True`` flips M for mixed items only; unmixed items stay unmixed.

    ``want_mask``: M itself, uint8 (B,H,W).  ``want_count``: ``mixed_count`` int64 (B,), the pixels with M = 1 (a memset, then one
    integer atomic per workgroup: exact and independent of order).  ``out``: a dict of dense tensors to fill under the results'
    names; an entry that shares memory with an input is refused (item b reads item ``partner[b]``: in-place use is a race).

    The outputs are bit copies of the inputs, NaN payloads included; inputs are never modified; non-dense inputs are made dense
    first (a copy by the tensor library).  Where W is a multiple of 4 and every base is 16-byte aligned a lane moves four pixels
    with 16-byte accesses, otherwise one.  No host read and every parameter in device memory: a launch plan can hold the call
    (``mix_launches``); two calls give the same bits.  Not differentiable: the results carry no graph."""
    check_mix_options(images, labels, partner, kind=kind, boxes=boxes, class_labels=class_labels, sel=sel, mask=mask, invert=invert,
                      pixel_weight=pixel_weight, scores=scores, want_mask=want_mask, want_count=want_count, out=out)
    dense = lambda t: None if t is None else t.detach().contiguous()          # noqa: E731
    images, labels, partner, pixel_weight, scores = (dense(t) for t in (images, labels, partner, pixel_weight, scores))
    boxes, class_labels, sel, mask = (dense(t) for t in (boxes, class_labels, sel, mask))
    B, _, H, W = images.shape
    out = out or {}

    def result(key, like=None, shape=None, dtype=None):
        t = out.get(key)
        if t is None:
            t = torch.empty_like(like) if like is not None else torch.empty(shape, dtype=dtype, device=images.device)
        return t
    res = {"images": result("images", images), "labels": result("labels", labels)}
    pairs = [(images, res["images"]), (labels, res["labels"])]
    for key, t in (("pixel_weight", pixel_weight), ("scores", scores)):
        res[key] = None
        if t is not None:
            res[key] = result(key, t)
            pairs.append((t, res[key]))
    res["mask"] = result("mask", shape=(B, H, W), dtype=torch.uint8) if want_mask else None
    res["mixed_count"] = result("mixed_count", shape=(B,), dtype=torch.int64) if want_count else None
    arr = (_MixTensor * len(pairs))()
    for i, (src, dst) in enumerate(pairs):
        arr[i].src, arr[i].dst = _p(src), _p(dst)
        arr[i].channels, arr[i].elem_bytes = (src.shape[1] if src.dim() == 4 else 1), src.element_size()
    check(lib().wsdl_mix_apply(C.cast(arr, C.c_void_p), len(pairs), _p(partner), MIX_KINDS[kind], _p(boxes),
                               0 if boxes is None else boxes.shape[1], _p(class_labels), _p(sel), _p(mask), int(invert), B, H, W,
                               _p(res["mask"]), _p(res["mixed_count"]), _stream()))
    return MixResult(**res)


# ---- score histograms: grouped histograms with exact counts, threshold sweeps, Otsu, calibration (csrc/score_hist.hip) -----------
HIST_MAX_BINS = 1024                                # WSDL_HIST_MAX_BINS
HIST_MAX_GROUPS = 32                                # WSDL_HIST_MAX_GROUPS
HIST_MAX_SLOTS = 4096                               # WSDL_HIST_MAX_SLOTS
CONFIDENCE_MAX_CLASSES = 64                         # WSDL_CONFIDENCE_MAX_CLASSES
OTSU_MAX_PIXELS = 1 << 21
HIST_SUM_SCALE = 16777216.0                         # the fixed point of ``sums``: 2^24
_EDGES_CACHE = {}


def _int_in(v, name, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise WsdlError(f"{name}: {what} {v!r} must be an int in [{lo}, {hi}]")
    return int(v)


def uniform_edges(lo, hi, bins, device=None):
    """``bins + 1`` equally spaced float32 edges from ``lo`` to ``hi``: ``np.linspace`` in float64, rounded once to float32.  On
    ``device`` (cached per (lo, hi, bins, device): a second call costs no copy) or, with ``device=None``, as a numpy array."""
    bins = _int_in(bins, "uniform_edges", "bins", 1, HIST_MAX_BINS)
    if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) for v in (lo, hi)) or not lo < hi:
        raise WsdlError(f"uniform_edges: range ({lo!r}, {hi!r}) must be two finite numbers, lo < hi")
    host = np.linspace(float(lo), float(hi), bins + 1, dtype=np.float64).astype(np.float32)
    if device is None:
        return host
    key = (float(lo), float(hi), bins, str(torch.device(device)))
    t = _EDGES_CACHE.get(key)
    if t is None:
        t = torch.from_numpy(host).to(device)
        t._wsdl_edges_host = (t._version, host)
        _EDGES_CACHE[key] = t
    return t


def _edges_host(edges):
    """The float32 host copy of an edges tensor; read from the device once per tensor and version."""
    tag = getattr(edges, "_wsdl_edges_host", None)
    if tag is not None and tag[0] == edges._version:
        return tag[1]
    host = np.ascontiguousarray(edges.detach().cpu().numpy())
    edges._wsdl_edges_host = (edges._version, host)
    return host


def check_score_hist_options(scores=None, groups=None, *, edges=None, bins=256, range=(0.0, 1.0), num_groups=1, per_image=True,
                             want_sums=False, out=None, counts=None, sums=None, curves=False, otsu_groups=None, fallback=0.5,
                             segment_pixels=0, thresh=None, logits=None, labels=None, ignore_index=-100, extra_outs=(),
                             name="score_histogram"):
    """Host-side validation shared by ``score_histogram``, ``threshold_curves``, ``otsu_threshold``, ``threshold_per_image`` and
    ``confidence_histogram``, before any device call; returns ``(G, nb, host copy of the edges or None)``.  WsdlError for:
    ``scores`` not a float32 tensor of rank >= 2 / with an empty dimension, ``groups`` not an int64 tensor of its shape; ``edges``
    not a one-dimensional float32 tensor of 2..1025 values, not finite or not strictly ascending, outside [-128, 128] with
    ``want_sums``; ``bins`` / ``range`` / ``num_groups`` outside the table limits (1024 bins, 32 groups, 4096 slots); a segment of
    2^31 pixels or more; ``counts`` / ``sums`` not dense int64 (S, G, nb + 3) tensors, ``G != 2`` where curves are asked for, an
    Otsu group outside [0, G), a non-finite ``fallback`` or an Otsu segment of more than 2^21 pixels; ``thresh`` neither a number nor a float32 (B,) tensor; ``logits`` /
    ``labels`` of the wrong rank, type, size or more than 64 classes; an output (``out`` entries, ``extra_outs``) that shares memory
    with an input or another output.  The place comes last: everything above is refused without a device."""
    tensors, inputs = [], []
    B = None

    def tensor(t, what, dtype, rank=None, min_rank=None, shape=None):
        if not torch.is_tensor(t):
            raise WsdlError(f"{name}: {what} must be a tensor")
        if rank is not None and t.dim() != rank or min_rank is not None and t.dim() < min_rank:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} must have rank {rank if rank is not None else '>= %d' % min_rank}")
        if t.dtype != dtype:
            raise WsdlError(f"{name}: {what} must be {dtype}, got {t.dtype}")
        if t.numel() == 0:
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} has an empty dimension")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise WsdlError(f"{name}: {what} {tuple(t.shape)} must be {tuple(shape)}")
        tensors.append((t, what))

    if not isinstance(per_image, (bool, np.bool_)) or not isinstance(want_sums, (bool, np.bool_)):
        raise WsdlError(f"{name}: per_image and want_sums must be bools")
    seg = None
    if scores is not None:
        tensor(scores, "scores", torch.float32, min_rank=2)
        inputs.append((scores, "scores"))
        B = scores.shape[0]
        if groups is not None:
            tensor(groups, "groups", torch.int64, shape=scores.shape)
            inputs.append((groups, "groups"))
        seg = scores.numel() // B if per_image else scores.numel()
    if logits is not None:
        tensor(logits, "logits", torch.float32, rank=4)
        B = logits.shape[0]
        if logits.shape[1] > CONFIDENCE_MAX_CLASSES:
            raise WsdlError(f"{name}: logits {tuple(logits.shape)}: at most {CONFIDENCE_MAX_CLASSES} classes")
        tensor(labels, "labels", torch.int64, shape=(B,) + tuple(logits.shape[2:]))
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
            raise WsdlError(f"{name}: ignore_index {ignore_index!r} must be an int")
        inputs += [(logits, "logits"), (labels, "labels")]
        seg = labels.numel() // B if per_image else labels.numel()
    if B is not None and B > 65535:
        raise WsdlError(f"{name}: {B} images, at most 65535")
    if seg is not None and seg >= 1 << 31:
        raise WsdlError(f"{name}: a segment of {seg} pixels, fewer than 2^31 are supported")
    host = None
    if edges is not None:
        tensor(edges, "edges", torch.float32, rank=1)
        inputs.append((edges, "edges"))
        nb = edges.numel() - 1
        if not 1 <= nb <= HIST_MAX_BINS:
            raise WsdlError(f"{name}: {edges.numel()} edges, 2..{HIST_MAX_BINS + 1} are supported")
        host = _edges_host(edges)
        if not np.isfinite(host).all():
            raise WsdlError(f"{name}: edges must be finite")
        if not (np.diff(host.astype(np.float64)) > 0).all():
            raise WsdlError(f"{name}: edges must be strictly ascending")
    elif counts is None and thresh is None:
        nb = _int_in(bins, name, "bins", 1, HIST_MAX_BINS)
        if (not isinstance(range, (tuple, list)) or len(range) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) or
                                                                          not np.isfinite(v) for v in range) or not range[0] < range[1]):
            raise WsdlError(f"{name}: range {range!r} must be two finite numbers (lo, hi), lo < hi")
        host = uniform_edges(range[0], range[1], nb)
        if not (np.diff(host.astype(np.float64)) > 0).all():
            raise WsdlError(f"{name}: range {range!r} has no {nb} distinct float32 bins")
    else:
        nb = None
    G = _int_in(num_groups, name, "num_groups", 1, HIST_MAX_GROUPS)
    if counts is not None:
        tensor(counts, "counts", torch.int64, rank=3)
        S, G, row = counts.shape
        if nb is None:
            nb = row - 3
        if row != nb + 3 or not 1 <= nb <= HIST_MAX_BINS:
            raise WsdlError(f"{name}: counts {tuple(counts.shape)} must be (S, G, bins + 3) with 1..{HIST_MAX_BINS} bins"
                            + ("" if edges is None else f" ({edges.numel()} edges given)"))
        if not counts.is_contiguous():
            raise WsdlError(f"{name}: counts must be dense")
        inputs.append((counts, "counts"))
        if sums is not None:
            tensor(sums, "sums", torch.int64, shape=counts.shape)
        if curves and G != 2:
            raise WsdlError(f"{name}: curves need counts of G = 2 groups (group 1 the positives), got G = {G}")
        if otsu_groups is not None:
            for g in otsu_groups:
                _int_in(g, name, "group", 0, G - 1)
            if len(list(otsu_groups)) == 0:
                raise WsdlError(f"{name}: groups selects nothing")
        if isinstance(fallback, bool) or not isinstance(fallback, (int, float)) or not np.isfinite(fallback):
            raise WsdlError(f"{name}: fallback {fallback!r} must be a finite number")
        if isinstance(segment_pixels, bool) or not isinstance(segment_pixels, int) or segment_pixels < 0:
            raise WsdlError(f"{name}: segment_pixels {segment_pixels!r} must be an int >= 0")
        if segment_pixels > OTSU_MAX_PIXELS:
            raise WsdlError(f"{name}: segments of {segment_pixels} pixels, at most 2^21 = {OTSU_MAX_PIXELS} are supported")
    if G > HIST_MAX_GROUPS or (nb is not None and G * (nb + 3) > HIST_MAX_SLOTS):
        raise WsdlError(f"{name}: {G} groups x ({nb} + 3) slots, at most {HIST_MAX_GROUPS} groups and {HIST_MAX_SLOTS} slots")
    if want_sums and host is not None and np.abs(host).max() > 128.0:
        raise WsdlError(f"{name}: want_sums needs every edge in [-128, 128]")
    if thresh is not None:
        if torch.is_tensor(thresh):
            tensor(thresh, "thresh", torch.float32, shape=(B,))
            inputs.append((thresh, "thresh"))
        elif isinstance(thresh, bool) or not isinstance(thresh, (int, float)):
            raise WsdlError(f"{name}: thresh {thresh!r} must be a number or a float32 (B,) tensor")
    outs = []
    if out is not None and not isinstance(out, dict):
        raise WsdlError(f"{name}: out must be a dict of tensors to fill")
    for what, t in list((out or {}).items()) + list(extra_outs):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.requires_grad:
            raise WsdlError(f"{name}: {what} must be a tensor that needs no gradient")
        for other, oname in inputs + outs:
            if _shares_memory(t, other):
                raise WsdlError(f"{name}: {what} shares memory with {oname}")
        outs.append((t, what))
        tensors.append((t, what))
    device = None                                   # the place last: everything above can be refused without a device
    for t, what in tensors:
        if not t.is_cuda:
            raise WsdlError(f"{name}: {what}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
        if device is None:
            device = t.device
        elif t.device != device:
            raise WsdlError(f"{name}: {what} is on {t.device}, the other tensors on {device}")
    return G, nb, host


def score_histogram(scores, groups=None, *, edges=None, bins=256, range=(0.0, 1.0), num_groups=1, per_image=True, want_sums=False,
                    out=None):
    """Grouped histogram of the float32 device planes ``scores`` (B, ...) with exact integer counts kept on the device
    (wsdl_score_hist).  ``groups``: int64 of the shape of ``scores`` or None (all group 0); a pixel whose group is outside
    ``[0, num_groups)`` is not counted (a trimap's 2, the void label 255).  ``edges``: ``nb + 1`` strictly ascending float32 values on
    the device, or None for ``uniform_edges(*range, bins)``.  Returns int64 ``counts`` (S, G, nb + 3), S = B with ``per_image`` else 1;
    the slots, defined by comparisons alone: 0: ``v < edges[0]``; ``1 + k``: ``edges[k] <= v < edges[k + 1]``; ``nb + 1``:
    ``v >= edges[nb]``; ``nb + 2``: NaN.  With ``want_sums`` also ``sums`` of the same shape: the sum of
    ``int64(v * 2^24)`` (exact product, truncated) over the pixels of the slots 1 .. nb - every edge must then lie in [-128, 128].
    ``out``: a dict whose dense ``"counts"`` / ``"sums"`` tensors are refilled (no stale counts: the call zeroes them).  Inputs are
    not modified; non-dense inputs are made dense first; no host read, bitwise reproducible, a launch plan can hold the call."""
    G, nb, host = check_score_hist_options(scores, groups, edges=edges, bins=bins, range=range, num_groups=num_groups,
                                           per_image=per_image, want_sums=want_sums, out=out)
    scores = scores.detach()
    scores = scores if scores.is_contiguous() else scores.contiguous()
    if groups is not None:
        groups = groups if groups.is_contiguous() else groups.contiguous()
    if edges is None:
        edges = uniform_edges(range[0], range[1], nb, scores.device)
    B = scores.shape[0]
    HW = scores.numel() // B
    S = B if per_image else 1
    counts = _out_tensor(out, "counts", (S, G, nb + 3), torch.int64, scores.device)
    sums = _out_tensor(out, "sums", (S, G, nb + 3), torch.int64, scores.device) if want_sums else None
    check(lib().wsdl_score_hist(_p(scores), _p(groups), _p(edges), host.ctypes.data, B, HW, G, nb, int(bool(per_image)), _p(counts),
                                _p(sums), _stream()))
    counts._wsdl_segment_pixels = HW if per_image else B * HW
    return (counts, sums) if want_sums else counts


def threshold_curves(counts, out=None):
    """From the ``counts`` (S, 2, nb + 3) of ``score_histogram`` with two groups - group 1 the positives - int64 ``curves``
    (S, nb + 1, 4) on the device: TP, FP, FN, TN of the prediction ``v >= edges[k]`` for k = 0 .. nb (wsdl_hist_curves).  NaN
    pixels and pixels below the first edge are never predicted positive.  ``out``: a dense int64 tensor to fill."""
    _G, nb, _ = check_score_hist_options(counts=counts, curves=True, extra_outs=[("out", out)], name="threshold_curves")
    S = counts.shape[0]
    if out is None or tuple(out.shape) != (S, nb + 1, 4) or out.dtype != torch.int64 or not out.is_contiguous():
        out = torch.empty(S, nb + 1, 4, device=counts.device, dtype=torch.int64)
    check(lib().wsdl_hist_curves(_p(counts), S, nb, _p(out), _stream()))
    return out


def otsu_threshold(counts, edges, groups=None, fallback=0.5, *, segment_pixels=None):
    """Otsu's threshold per segment from ``counts`` (S, G, nb + 3) over the bins 1 .. nb of the groups ``groups`` (ints; None: all),
    on the device (wsdl_otsu).  With h_i the bin counts, for k = 0 .. nb - 2: ``w0 = sum_{i<=k} h_i``, ``w1 = N - w0``,
    ``s0 = sum_{i<=k} i h_i``, ``s1 = S - s0``, ``D = s0 w1 - s1 w0`` (int64), ``q(k) = (float64(D) * float64(D)) / float64(w0 w1)``
    where ``w0 w1 > 0``.  Returns ``(k, threshold, q)``: int32 ``k*`` = the first maximum of q, float32 ``edges[k* + 1]`` (pixels
    with ``v >= threshold`` are foreground) and float64 ``q(k*)``; with fewer than two occupied bins ``k* = -1``, the threshold is
    ``fallback`` and q is 0.  Segments of more than 2^21 pixels are refused (D must stay below 2^53): the size is what
    ``score_histogram`` recorded for ``counts``, or ``segment_pixels``; a segment that holds more all the same gets ``k* = -2`` and
    NaN.  Equal to the same formula in numpy float64 bit for bit."""
    npix = segment_pixels if segment_pixels is not None else getattr(counts, "_wsdl_segment_pixels", 0)
    G, nb, _ = check_score_hist_options(counts=counts, edges=edges, otsu_groups=groups, fallback=fallback, segment_pixels=npix,
                                        name="otsu_threshold")
    mask = (1 << G) - 1 if groups is None else sum(1 << g for g in set(int(g) for g in groups))
    S = counts.shape[0]
    dev = counts.device
    k = torch.empty(S, device=dev, dtype=torch.int32)
    thr = torch.empty(S, device=dev, dtype=torch.float32)
    q = torch.empty(S, device=dev, dtype=torch.float64)
    check(lib().wsdl_otsu(_p(counts), _p(edges), S, G, nb, mask, float(fallback), npix, _p(k), _p(thr), _p(q), _stream()))
    return k, thr, q


def threshold_per_image(scores, thresh, positive_only=True, want_count=False, out=None):
    """uint8 ``mask[b, ...] = scores[b, ...] >= thresh[b]``, with ``positive_only`` (the LayerCAM epilogue's rule) also
    ``scores > 0`` (wsdl_threshold_images).  ``scores``: float32 device planes (B, ...); ``thresh``: a float32 (B,) device tensor -
    what ``otsu_threshold`` returns - or a number; a NaN threshold gives an empty mask.  ``want_count``: also the int64 (B,) number
    of set pixels, from the same launch.  ``out``: a dict whose ``"mask"`` / ``"count"`` tensors are filled.  No host read."""
    check_score_hist_options(scores, thresh=thresh, out=out, name="threshold_per_image")
    scores = scores.detach()
    scores = scores if scores.is_contiguous() else scores.contiguous()
    B = scores.shape[0]
    if not torch.is_tensor(thresh):
        thresh = torch.full((B,), float(thresh), device=scores.device, dtype=torch.float32)
    thresh = thresh if thresh.is_contiguous() else thresh.contiguous()
    mask = _out_tensor(out, "mask", tuple(scores.shape), torch.uint8, scores.device)
    count = _out_tensor(out, "count", (B,), torch.int64, scores.device) if want_count else None
    check(lib().wsdl_threshold_images(_p(scores), _p(thresh), B, scores.numel() // B, int(bool(positive_only)), _p(mask), _p(count),
                                      _stream()))
    return (mask, count) if want_count else mask


def confidence_histogram(logits, labels, bins=15, ignore_index=-100, per_image=False, conf_out=None, pred_out=None):
    """The reliability table of a classifier's float32 device logits (B,C,H,W), C <= 64, against int64 labels (B,H,W)
    (wsdl_confidence_hist).  Per pixel ``pred`` = the first class of largest logit and ``conf`` = the softmax maximum, taken in
    double and rounded once to float32 (NaN where a logit is not finite: the NaN slot); a pixel with ``label != ignore_index`` is
    counted in group ``(pred == label)`` of a two-group histogram over ``bins`` uniform edges on [0, 1].  Returns ``(counts, sums)``
    as ``score_histogram(..., want_sums=True)`` does, (S, 2, bins + 3) with S = B for ``per_image`` else 1.  ``conf_out`` /
    ``pred_out``: dense float32 / int64 (B,H,W) tensors that receive the two planes (every pixel).  No host read."""
    check_score_hist_options(logits=logits, labels=labels, ignore_index=ignore_index, bins=bins, range=(0.0, 1.0), num_groups=2,
                             per_image=per_image, want_sums=True, extra_outs=[("conf_out", conf_out), ("pred_out", pred_out)],
                             name="confidence_histogram")
    logits = logits.detach()
    logits = logits if logits.is_contiguous() else logits.contiguous()
    labels = labels if labels.is_contiguous() else labels.contiguous()
    B, Cc, H, W = logits.shape
    for t, what, dtype in ((conf_out, "conf_out", torch.float32), (pred_out, "pred_out", torch.int64)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (B, H, W) or not t.is_contiguous()):
            raise WsdlError(f"confidence_histogram: {what} must be a dense {dtype} {(B, H, W)} tensor")
    edges = uniform_edges(0.0, 1.0, bins, logits.device)
    S = B if per_image else 1
    counts = torch.empty(S, 2, bins + 3, device=logits.device, dtype=torch.int64)
    sums = torch.empty_like(counts)
    check(lib().wsdl_confidence_hist(_p(logits), _p(labels), _p(edges), _edges_host(edges).ctypes.data, B, Cc, H, W, int(ignore_index),
                                     bins, int(bool(per_image)), _p(counts), _p(sums), _p(conf_out), _p(pred_out), _stream()))
    counts._wsdl_segment_pixels = H * W if per_image else B * H * W
    return counts, sums


# host-side float64 reductions of the (tiny) count tensors: numpy, no kernels
def _np64(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def _ratio(num, den, empty):
    num, den = np.broadcast_arrays(np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), empty)


def iou_curve_from_counts(curves, empty=1.0, eps=0.0):
    """IoU of the foreground per threshold from ``curves`` (..., 4) = TP FP FN TN: ``TP / (TP + FP + FN)`` in float64, ``empty``
    where the union is 0.  ``eps > 0``: ``TP / (union + eps)`` at every entry instead - ``compute_iou_and_acc``'s expression, which
    gives 0 for an empty union."""
    c = _np64(curves)
    union = c[..., 0] + c[..., 1] + c[..., 2]
    return c[..., 0] / (union + eps) if eps > 0 else _ratio(c[..., 0], union, empty)


def accuracy_curve_from_counts(curves):
    """Pixel accuracy per threshold: ``(TP + TN) / (TP + FP + FN + TN)``, 0 for an empty segment."""
    c = _np64(curves)
    return _ratio(c[..., 0] + c[..., 3], c.sum(axis=-1), 0.0)


def _fbeta_curve(c, beta2):
    return _ratio((1.0 + beta2) * c[..., 0], (1.0 + beta2) * c[..., 0] + beta2 * c[..., 2] + c[..., 1], 0.0)


def best_threshold(curves, edges, metric="iou", reduce="dataset", beta2=0.3):
    """The threshold of best ``metric`` ('iou' | 'f', the F-measure with ``beta2``) from ``curves`` (S, nb + 1, 4):
    ``reduce='dataset'`` pools the counts of the segments first, 'mean_image' averages the per-segment metric.  Returns
    ``(threshold, value, k)``: the first maximum."""
    if metric not in ("iou", "f") or reduce not in ("dataset", "mean_image"):
        raise WsdlError(f"best_threshold: metric {metric!r} ('iou' | 'f'), reduce {reduce!r} ('dataset' | 'mean_image')")
    c, e = _np64(curves), _np64(edges)
    c = c.reshape((-1,) + c.shape[-2:])
    if c.shape[1] != e.shape[0]:
        raise WsdlError(f"best_threshold: curves {c.shape} do not belong to {e.shape[0]} edges")
    if reduce == "dataset":
        c = c.sum(axis=0, keepdims=True)
    m = (iou_curve_from_counts(c) if metric == "iou" else _fbeta_curve(c, beta2)).mean(axis=0)
    k = int(np.argmax(m))
    return float(e[k]), float(m[k]), k


def pr_curve(curves):
    """``(precision, recall)`` per threshold from pooled ``curves`` (..., nb + 1, 4): TP / (TP + FP), 1 where nothing is predicted,
    and TP / (TP + FN), 0 where there is no positive."""
    c = _np64(curves)
    c = c.reshape((-1,) + c.shape[-2:]).sum(axis=0)
    return _ratio(c[:, 0], c[:, 0] + c[:, 1], 1.0), _ratio(c[:, 0], c[:, 0] + c[:, 2], 0.0)


def average_precision(curves):
    """Area under the precision-recall steps of ``pr_curve``: ``sum_k (R_k - R_{k+1}) P_k`` with the thresholds ascending and
    ``R_{nb+1} = 0``.  Positives below the first edge are never recalled."""
    p, r = pr_curve(curves)
    return float(np.sum((r - np.append(r[1:], 0.0)) * p))


def max_fbeta(curves, beta2=0.3):
    """``(F_max, k)``: the maximum over the thresholds of ``(1 + beta2) P R / (beta2 P + R)`` from the pooled ``curves``, and the
    first threshold index that reaches it (beta2 = 0.3: the saliency literature's F-measure)."""
    c = _np64(curves)
    f = _fbeta_curve(c.reshape((-1,) + c.shape[-2:]).sum(axis=0), beta2)
    k = int(np.argmax(f))
    return float(f[k]), k


def _pooled_bins(counts, sums, hi):
    """Per group (2, nb): pixel counts and value sums of the bins; the slot above the last edge joins the last bin at value ``hi``."""
    c, s = _np64(counts), _np64(sums) / HIST_SUM_SCALE
    c, s = c.reshape((-1,) + c.shape[-2:]).sum(axis=0), s.reshape((-1,) + s.shape[-2:]).sum(axis=0)
    n, v = c[:, 1:-2].copy(), s[:, 1:-2].copy()
    n[:, -1] += c[:, -2]
    v[:, -1] += c[:, -2] * hi
    return c, n, v


def mae_from_sums(counts, sums, lo=0.0, hi=1.0):
    """Mean absolute error of a score map against the binary ground truth its two groups encode (group 1: target 1), from the
    ``(counts, sums)`` of ``score_histogram(..., num_groups=2, want_sums=True)`` over [lo, hi]: values outside the range count as
    clamped to it, NaN pixels are left out."""
    c, n, v = _pooled_bins(counts, sums, hi)
    v[:, 0] += c[:, 0] * lo
    n[:, 0] += c[:, 0]
    total = n.sum()
    return float((v[0].sum() + (n[1].sum() - v[1].sum())) / total) if total else 0.0


def ece_from_counts(counts, sums):
    """Expected calibration error from the ``(counts, sums)`` of ``confidence_histogram`` (pooled over the segments):
    ``(ece, accuracy, mean confidence, count)`` with one entry per bin; a confidence of exactly 1 belongs to the last bin; empty
    bins have NaN accuracy and confidence and weigh nothing."""
    _c, n, v = _pooled_bins(counts, sums, 1.0)
    cnt = n[0] + n[1]
    acc, conf = _ratio(n[1], cnt, np.nan), _ratio(v[0] + v[1], cnt, np.nan)
    total = cnt.sum()
    ece = float(np.sum(np.where(cnt > 0, cnt * np.abs(np.where(cnt > 0, acc - conf, 0.0)), 0.0)) / total) if total else 0.0
    return ece, acc, conf, cnt.astype(np.int64)


def tau_for_precision(counts, edges, target):
    """The smallest edge at and above which the pooled accuracy of ``confidence_histogram``'s counts is at least ``target``; None
    where no edge with a pixel at or above it qualifies."""
    c, e = _np64(counts), _np64(edges)
    c = c.reshape((-1,) + c.shape[-2:]).sum(axis=0)
    right = np.cumsum(c[1, 1:-1][::-1])[::-1]
    both = np.cumsum((c[0, 1:-1] + c[1, 1:-1])[::-1])[::-1]
    for k in np.arange(e.shape[0]):
        if both[k] > 0 and right[k] / both[k] >= target:
            return float(e[k])
    return None


def softmax_channels(x):
    return _SoftmaxChannels.apply(x)


class _SoftmaxChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dense(x, "x")
        B, Cc = x.shape[0], x.shape[1]
        HW = x.numel() // (B * Cc)
        y = torch.empty_like(x)
        check(lib().wsdl_softmax_fwd(_p(x), _p(y), B, Cc, HW, _stream()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _dense(dy, "dy")
        B, Cc = y.shape[0], y.shape[1]
        dx = torch.empty_like(y)
        check(lib().wsdl_softmax_bwd(_p(y), _p(dy), _p(dx), B, Cc, y.numel() // (B * Cc), _stream()))
        return dx


class _KLDivBatchMean(torch.autograd.Function):
    """F.kl_div((xn + 1e-8).log(), s, reduction='batchmean') and d/dxn."""

    @staticmethod
    def forward(ctx, xn, s):
        xn, s = _dense(xn, "xn"), _dense(s, "s")
        loss = torch.empty((), device=xn.device, dtype=torch.float32)
        dxn = torch.empty_like(xn)
        ws = workspace(lib().wsdl_reduce_workspace(), xn.device)
        check(lib().wsdl_kl_div_fwd_bwd(_p(xn), _p(s), _p(loss), _p(dxn), xn.numel(), xn.shape[0], _p(ws), ws.numel(),
                                        _stream()))
        ctx.save_for_backward(dxn)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dxn,) = ctx.saved_tensors
        out = torch.empty_like(dxn)
        check(lib().wsdl_scale_by_device_scalar(_p(dxn), _p(_dense(g.reshape(1))), _p(out), dxn.numel(), _stream()))
        return out, None


class _ScaleMean(torch.autograd.Function):
    """w * mean(x) of a device scalar / vector as launches of the library (a launch plan sees them; ``0.1 * loss`` and
    ``.mean()`` are kernels of the tensor library)."""

    @staticmethod
    def forward(ctx, x, w):
        xs = _dense(x, "x")
        out = torch.empty((), device=x.device, dtype=torch.float32)
        check(lib().wsdl_scale_mean(_p(xs), xs.numel(), float(w), _p(out), _stream()))
        ctx.w, ctx.shape = float(w), tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        n = 1
        for d in ctx.shape:
            n *= d
        dx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib().wsdl_scale_fill(_p(_dense(g.reshape(1))), ctx.w / n, _p(dx), n, _stream()))
        return dx, None


def scale_mean(x, w=1.0):
    """``w * x.mean()`` (``w * x`` for a scalar) -> 0-dim tensor."""
    return _ScaleMean.apply(x, float(w))


class _Fanout(torch.autograd.Function):
    """n handles on one tensor whose gradients are summed by the library's add kernel, in the order of the handles.  A tensor
    consumed twice has its gradients added by the autograd engine with a kernel of the tensor library - which a launch plan
    does not see (the logits feeding the cross-entropy AND a pairwise loss)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        outs = tuple(_alias(x) for _ in range(n))
        a = getattr(x, "_wsdl_amax", None)
        if a is not None and getattr(x, "_wsdl_amax_version", x._version) == x._version:
            for o in outs:
                _publish_amax(o, a)
        return outs

    @staticmethod
    def backward(ctx, *gs):
        gs = [_dense(g, "gradient") for g in gs if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            return gs[0], None
        acc = torch.empty_like(gs[0])
        check(lib().wsdl_add(_p(gs[0]), _p(gs[1]), _p(acc), acc.numel(), 0, _stream()))
        for g in gs[2:]:
            check(lib().wsdl_add(_p(acc), _p(g), _p(acc), acc.numel(), 0, _stream()))
        return acc, None


def fanout(x, n=2):
    """``n`` handles on ``x`` for ``n`` consumers (see _Fanout); without autograd just ``x`` n times."""
    if not (torch.is_grad_enabled() and x.requires_grad and x.is_cuda):
        return (x,) * n
    return _Fanout.apply(x, int(n))


def add_scalars(a, b):
    """a + b for two 0-dim device tensors through the library's add kernel."""
    return _AddAct.apply(a.reshape(1), b.reshape(1), False).reshape(())


def kl_div_batchmean(xn, s):
    return _KLDivBatchMean.apply(xn, s)


# ---- profiler ranges (roctx): WSDL_ROCTX=1 in the environment (or ranges_enable(True)) brackets the phases of a training step
# and of a CAM batch, and every instrumented kernel class, with named ranges for `rocprofv3 --marker-trace`
RANGES = [False]


def ranges_enable(on=True):
    check(lib().wsdl_range_enable(int(bool(on))))
    RANGES[0] = bool(on)


class prof_range:
    """``with ops.prof_range("backward"): ...`` - a named roctx range when ranges are enabled, nothing otherwise."""
    __slots__ = ("name",)

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if RANGES[0]:
            lib().wsdl_range_push(self.name.encode())

    def __exit__(self, *exc):
        if RANGES[0]:
            lib().wsdl_range_pop()
        return False


if os.environ.get("WSDL_ROCTX") == "1":
    try:
        ranges_enable(True)
    except Exception:           # the profiler SDK is not there: run without ranges
        RANGES[0] = False


PROF_ON = [False]      # per-launch event brackets are being recorded (bench.py's roofline pass): a plan replay has none


def prof_enable(on):
    check(lib().wsdl_prof_enable(int(on)))
    PROF_ON[0] = bool(on)


def prof_reset():
    check(lib().wsdl_prof_reset())


PROF_NCLASSES = 23


def prof_class_name(cls):
    return lib().wsdl_prof_class_name(int(cls)).decode()


def prof_collect(cls):
    n, ms, work, exe, byt = C.c_longlong(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
    check(lib().wsdl_prof_collect(int(cls), C.byref(n), C.byref(ms), C.byref(work), C.byref(exe), C.byref(byt)))
    return n.value, ms.value, work.value, exe.value, byt.value
