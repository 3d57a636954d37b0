"""Range slots of the f16 matrix-core kernels (include/rave_hip.h, csrc/common.hpp: RH_X6_F16; armed by _arming.armed_call).

The x6 kernels scale every activation operand by a power of two derived from the TENSOR's max |x|.  That maximum travels with
the tensor as a "range slot" (kRangeWords uint32 in device memory): the kernel that produces a tensor leaves it there
(epilogue atomicMax: no extra pass), and the tensor OBJECT carries the slot as an attribute together with its version
counter (RangeTag).  A tensor without a (current) slot -- produced by a torch op, a view, modified in place -- gets one from a
pass of rh_amax_f32 the first time a convolution consumes it.  Slots come from a zeroed pool; RAVE.training_step takes a fresh
pool per step (range_reset: one fill launch -- recorded into a hipGraph it re-zeroes the slots at every replay, so a replayed
step computes the same scales as an eager one).  A pool taken inside a capture belongs to the graph (every replay re-zeroes it):
eager work after the capture never takes a slot from it (_new_range starts a fresh pool; GraphedTrainingStep also drops it from
the table when the recording ends and keeps it alive with the graph, range_capture_end).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from ._side import SIDE

Tensor = torch.Tensor

_RANGES = L.lib.rh_x6_uses_ranges() == 1
_RANGE_WORDS = L.lib.rh_x6_range_words()
_RANGE_SLOTS = 2048     # 4 KB each: more than any step of the shipped configs uses (a pool that runs out mid-step is replaced)


class RangePool:
    """The slot pool of one device."""
    __slots__ = ("pool", "cursor", "previous", "reset_stream", "captured")

    def __init__(self, pool, previous, reset_stream, captured):
        self.pool = pool                     # _RANGE_SLOTS x _RANGE_WORDS int32, zeroed
        self.cursor = 0                      # the next slot to hand out
        self.previous = previous             # the pool before this one (kept alive: a side stream may still read it)
        self.reset_stream = reset_stream     # stream of the reset
        self.captured = captured             # taken inside a stream capture


class RangeTag(NamedTuple):
    """``t._rh_range``: the slot of tensor ``t``, valid while ``t._version == version``.  ``origin`` = (stream, captured, event)
    of a slot that rh_amax_f32 filled on the weight-gradient side stream (_valid_slot)."""
    slot: Tensor
    version: int
    origin: Optional[tuple] = None


_RANGE_POOLS = {}        # device -> RangePool


def range_reset(device=None, _exhausted: bool = False) -> None:
    """Start a fresh zeroed slot pool (call at the start of a step; mandatory inside a hipGraph capture)."""
    if not _RANGES:
        return
    for dev in ([device] if device is not None else list(_RANGE_POOLS)):
        st = _RANGE_POOLS.get(dev)
        prev = st.pool if st else None
        cur = torch.cuda.current_stream(dev)
        pool = torch.zeros(_RANGE_SLOTS * _RANGE_WORDS, device=dev, dtype=torch.int32)
        if _exhausted:
            # a pool that ran out in the middle of a step, possibly on the weight-gradient side stream: the other stream of the
            # step must not publish into the new pool before its zero fill has run
            ev = torch.cuda.Event()
            ev.record(cur)
            d_ = dev if isinstance(dev, torch.device) else torch.device(dev)
            for other in [st.reset_stream if st else None,
                          SIDE.streams.get(d_.index if d_.index is not None else torch.cuda.current_device())]:
                if other is not None and other != cur:
                    other.wait_event(ev)
            main = st.reset_stream if st else cur
        else:
            main = cur
        _RANGE_POOLS[dev] = RangePool(pool, prev, main, torch.cuda.is_current_stream_capturing())


def range_capture_end(device=None) -> list:
    """Call when a stream capture has ended (successfully or not): the pools taken inside it are dropped from the table, so that
    no later eager launch takes a slot that the graph's replays re-zero (or, before the first replay, that was never zeroed).
    Returns them: the caller keeps them alive as long as the graph exists."""
    out = []
    for dev in ([device] if device is not None else list(_RANGE_POOLS)):
        st = _RANGE_POOLS.get(dev)
        if st is not None and st.captured:
            out += [t for t in (st.pool, st.previous) if t is not None]
            del _RANGE_POOLS[dev]
    return out


def _ranges_on() -> bool:
    return _RANGES and os.environ.get("RH_CONV_X6", "1") != "0"


def _new_range(device) -> Tensor:
    st = _RANGE_POOLS.get(device)
    if st is not None and st.captured and not torch.cuda.is_current_stream_capturing():
        range_reset(device)           # the pool of a finished capture (range_capture_end was not called): never handed out eagerly
        st = _RANGE_POOLS[device]
    if st is None or st.cursor >= _RANGE_SLOTS:
        range_reset(device, _exhausted=st is not None)
        st = _RANGE_POOLS[device]
    i = st.cursor
    st.cursor = i + 1
    return st.pool[i * _RANGE_WORDS:(i + 1) * _RANGE_WORDS]


def _attach_range(t: Optional[Tensor], slot: Optional[Tensor]) -> None:
    if t is not None and slot is not None:
        t._rh_range = RangeTag(slot, t._version)


def _reattach_range(t: Optional[Tensor], tag: Optional[RangeTag]) -> None:
    """Backward of a node that saved ``t``: put back the tag ``t`` carried in forward (the saved tensor may come back as a new
    object)."""
    if tag is not None and getattr(t, "_rh_range", None) is None:
        t._rh_range = tag


_RANGE_MISS = None       # diagnostics (range_miss_log_begin): [(tag, shape)] of the tensors that needed an rh_amax_f32 pass


def range_miss_log_begin() -> None:
    global _RANGE_MISS
    _RANGE_MISS = []


def range_miss_log_end():
    global _RANGE_MISS
    out, _RANGE_MISS = _RANGE_MISS, None
    return out


def _stream_of(handle, device) -> torch.cuda.Stream:
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream == handle:
        return cur
    for st in SIDE.streams.values():
        if st.cuda_stream == handle:
            return st
    return torch.cuda.ExternalStream(handle, device=device)


def _valid_slot(t: Tensor, s):
    """The slot attached to ``t`` if it is current, for a consumer on stream ``s``.  A slot that rh_amax_f32 filled on ANOTHER
    stream (the weight-gradient side stream, a weight gradient's operands under _OnSide) carries the event recorded right behind
    that pass: a consumer on a different stream waits for it (for the pass only, not for the weight-gradient kernels queued
    after it).  Such a slot filled inside a stream capture is not used outside it (and vice versa: an eager one inside a capture
    needs no wait -- the pass was queued before the recording)."""
    r = getattr(t, "_rh_range", None)
    if r is None or r.version != t._version or r.slot.device != t.device:
        return None
    if r.origin is not None and r.origin[0] != s:
        _, captured, ev = r.origin
        now = torch.cuda.is_current_stream_capturing()
        if captured and not now:
            return None
        if captured == now:
            _stream_of(s, t.device).wait_event(ev)
    return r.slot


def _range_of(t: Tensor, s, tag: str = "") -> Tensor:
    """The range slot of ``t``: the one its producer left -- also through a view that covers the whole producer tensor (same
    elements, same maximum; views share the version counter) --, else computed now (one pass over ``t`` on stream ``s``).
    The contract rests on the version counter: a write that bypasses it -- through ``.data``, or raw (ctypes / C ABI) writes
    into an existing tensor -- leaves a stale slot behind and is outside it (a bigger stale maximum costs accuracy, a smaller
    one overflows the f16 pieces)."""
    slot = _valid_slot(t, s)
    if slot is not None:
        return slot
    base = t._base
    if base is not None and base.numel() == t.numel():
        slot = _valid_slot(base, s)
        if slot is not None:
            t._rh_range = RangeTag(slot, t._version, base._rh_range.origin)
            return slot
    if _RANGE_MISS is not None:
        _RANGE_MISS.append((tag, tuple(t.shape)))
    slot = _new_range(t.device)
    L.check(L.lib.rh_amax_f32(L.ptr(t), t.numel(), L.ptr(slot), s), "amax")
    _attach_range(t, slot)
    side = next((st for st in SIDE.streams.values() if st.cuda_stream == s), None)
    if side is not None:
        # filled on the side stream: a consumer on the compute stream must not read it before this pass has run (_valid_slot)
        ev = torch.cuda.Event()
        ev.record(side)
        t._rh_range = RangeTag(slot, t._version, (s, torch.cuda.is_current_stream_capturing(), ev))
    return slot
