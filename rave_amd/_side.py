"""Weight-gradient branch of the backward pass on a side stream.

In the backward pass the weight-gradient branch of a layer (wgrad kernel -> ordered reduction of its K-slice partials ->
weight-norm backward: one MFMA kernel with a bandwidth-bound store tail, then two small bandwidth-bound kernels -- the
last of them collected over all layers of the branch into one launch at the join, SideBranch.wn below) only
feeds the optimizer, while the data-gradient chain is what the next layer waits for.  The branch (RH_BWD_SIDE_STREAM=0
disables) is enqueued on a second HIP stream: it forks after the kernels that produce its operands and is joined back (a) at the
end of the backward pass (autograd final callback) and (b) before a data-parallel bucket leaves (rave_amd.ddp).  Recorded
into the step's hipGraph the two streams become parallel branches of the graph.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import torch

from . import _lib as L


def _env(name: str, default=None):
    """The environment switches of the branch (RH_BWD_SIDE_STREAM, RH_WN_BATCH, RH_WN_BATCH_MAX, RH_REDUCE_BATCH, RH_SIDE_HOLD)."""
    return os.environ.get(name, default)


def _side_enabled() -> bool:
    return _env("RH_BWD_SIDE_STREAM", "1") != "0"


# Weight-norm backward of the layers whose weight gradient ran on the side stream: collected (SideBranch.wn) and run as ONE launch
# (rh_weight_norm_bwd_batched_f32) when the branch is joined -- at the end of the backward pass or when a data-parallel
# bucket leaves -- instead of one 4-6 us latency-bound launch per layer (56 per v2 step).  The dv / dg tensors handed to
# autograd are filled by that launch: like every gradient of the side stream they are valid once the branch is joined.
# RH_WN_BATCH=0: one launch per layer, at once.
_WN_BATCH_MAX = int(_env("RH_WN_BATCH_MAX", "64"))      # layers per launch (= the table size of the kernel): a pass with more pending layers launches early, on the side stream.
#                         (16 / 8 per launch -- so that only the last, small layers are left for the join -- measured the same
#                         step time as one launch at the join: 10.18-10.24 vs 10.16-10.20 ms)


def _wn_batch_enabled() -> bool:
    return _env("RH_WN_BATCH", "1") != "0"


# The ordered reductions of the weight gradients' K-slice partials, collected the same way (round 6: 56 launches of 9 - 15 us per
# v2 step, one behind every split weight-gradient kernel of the side stream): a weight-gradient call of the side stream leaves its
# partials in a scratch of its own (the ``defer`` item of _arming.armed_call) and every RH_REDUCE_BATCH layers -- and whenever the
# gradients are needed: the collected weight-norm launch, a data-parallel bucket, the join -- ONE launch reduces them all, each in
# the order its own launch would have used (bit-identical; RH_REDUCE_BATCH=0: one launch per layer, at once).
_RED_BATCH = 8


def _reduce_batch() -> int:
    """Layers per batched reduction; 0 = one launch per layer.  Default: 8 while a hipGraph is being recorded, 0 in eager steps --
    there the per-layer scratch allocation and the extra calls cost more host time than the launches they save (measured: the
    eager v2 step 9.5 -> 11.1 ms with batching, the replayed step unchanged at 232 instead of 281 dispatches).
    RH_REDUCE_BATCH=n forces n in both modes (read per call: tests)."""
    e = _env("RH_REDUCE_BATCH")
    if e is not None:
        return int(e)
    return _RED_BATCH if torch.cuda.is_current_stream_capturing() else 0


def _graph_task_id() -> int:
    """Id of the autograd graph task (backward pass) this thread is executing, -1 outside one."""
    f = getattr(torch._C, "_current_graph_task_id", None)
    return int(f()) if f is not None else -1


class _Pending(NamedTuple):
    """A branch that has forked and not yet been joined."""
    main: torch.cuda.Stream
    side: torch.cuda.Stream
    task: int           # the autograd graph task (backward pass) that queued the join


class SideBranch:
    """The state of the branch, one per process."""

    def __init__(self):
        self.streams = {}       # device index -> the side stream of that device
        self.pending = None     # _Pending
        self.hold = []          # incoming gradient tensors the branch still reads (see _OnSide): released when the branch is joined
        self.wn = []            # (dw, v, g, norms, dv, dg) of the collected weight-norm backward
        self.red = []           # (ReduceItem, scratch tensor, dw tensor): the tensors are kept alive until the batch has been launched

    def stream(self, device):
        """The stream of the weight-gradient branch of the backward pass (one per device)."""
        k = device.index if device.index is not None else torch.cuda.current_device()
        st = self.streams.get(k)
        if st is None:
            st = self.streams[k] = torch.cuda.Stream(device=device)
        return st

    def flush_reduce(self, stream_ptr) -> None:
        items, self.red[:] = list(self.red), []
        if not items:
            return
        arr = (L.ReduceItem * len(items))()
        for a, (it, _, _) in zip(arr, items):
            a.part, a.out, a.n, a.Z = it.part, it.out, it.n, it.Z
        L.check(L.lib.rh_reduce_partials_batched_f32(arr, len(items), stream_ptr), "reduce_partials_batched")

    def flush(self, stream_ptr) -> None:
        self.flush_reduce(stream_ptr)        # (the weight-norm backward reads the reduced gradients)
        items, self.wn[:] = list(self.wn), []
        if not items:
            return
        arr = (L.WnBwdItem * len(items))()
        for a, (dw, v, g, norms, dv, dg) in zip(arr, items):
            a.dw, a.v, a.g, a.norms, a.dv, a.dg = L.ptr(dw), L.ptr(v), L.ptr(g), L.ptr(norms), L.ptr(dv), L.ptr(dg)
            a.rows = v.shape[0]
            a.cols = v.numel() // max(v.shape[0], 1)
        L.check(L.lib.rh_weight_norm_bwd_batched_f32(arr, len(items), stream_ptr), "weight_norm_bwd_batched")

    def _flush_on_side(self, side) -> None:
        if self.wn or self.red:
            with torch.cuda.stream(side):
                self.flush(L.stream())

    def stream_for_collective(self, device):
        """Data-parallel bucket leaving while the backward pass still runs (rave_amd.ddp.GradReducer._launch): returns the stream
        the bucket's all-reduce must be ISSUED FROM so that it is ordered behind every gradient written so far -- the
        weight-gradient side stream, after the collected weight-norm launch of the branch has been enqueued there and after it
        has been made to wait for the calling (compute) stream -- or None when the branch has nothing in flight.  The compute
        stream itself is NOT made to wait: the data-gradient chain keeps running while the branch finishes and the collective
        starts (round 4 joined the branch into the compute stream at every bucket boundary)."""
        if self.pending is None:
            return None
        side = self.pending.side
        self._flush_on_side(side)
        side.wait_stream(torch.cuda.current_stream(device))
        return side

    def join(self) -> None:
        """The calling stream waits for everything enqueued on the weight-gradient side stream (after the collected
        weight-norm backward launches of that branch have been enqueued there)."""
        if self.pending is not None:
            main, side, _ = self.pending
            self._flush_on_side(side)
            main.wait_stream(side)
            torch.cuda.current_stream().wait_stream(side)
            self.pending = None
            self.hold.clear()

    def abandon(self, rejoin: bool = False) -> None:
        """Forget the side-stream bookkeeping of a pass that will never be joined (a step whose graph capture was refused midway):
        no kernel is launched -- the work recorded so far dies with the capture.  rejoin: the calling stream waits for the side
        streams first, so that a stream capture that forked onto them can be ended."""
        if rejoin:
            cur = torch.cuda.current_stream()
            for st in self.streams.values():
                try:
                    cur.wait_stream(st)
                except Exception:             # noqa: BLE001 -- a side stream that never joined the capture
                    pass
        self.pending = None
        self.hold.clear()
        self.wn.clear()
        self.red.clear()


SIDE = SideBranch()
_side_stream = SIDE.stream
side_stream_for_collective = SIDE.stream_for_collective
join_side_streams = SIDE.join
abandon_side_streams = SIDE.abandon


def _note_use(ctx, *params) -> None:
    """Forward side of the "exactly one pending use" rule of the side stream: a parameter that enters two nodes of one
    graph gets its two gradients ADDED by autograd on the compute stream -- which must not happen to a tensor the side
    stream is still writing.  Every differentiable use bumps a counter on the parameter, every backward takes it down."""
    ps = [p for p in params if p is not None and p.requires_grad]
    for p in ps:
        p._rh_pending = getattr(p, "_rh_pending", 0) + 1
        if p._rh_pending > 1:
            p._rh_shared = True          # stays set until every pending use has been taken down
    ctx.rh_params = ps


def _single_use(ctx) -> bool:
    """Backward side: True iff every parameter of this node has exactly this one pending use and no gradient yet (then the
    gradient returned here is adopted by autograd without being read).  Always takes the counters down."""
    ok = True
    for p in getattr(ctx, "rh_params", ()):
        n = getattr(p, "_rh_pending", 1)
        ok = ok and n == 1 and not getattr(p, "_rh_shared", False)
        # an EXISTING gradient (accumulation over several backward() calls, zero_grad(set_to_none=False), the other
        # optimizer's parameters in a GAN step) is accumulated into by AccumulateGrad on the COMPUTE stream -- it must not
        # read a tensor the side stream is still writing; likewise the data-parallel hook copies a gradient
        # into its bucket view on the compute stream when the view was not the one written (slot active but not fresh)
        if p.grad is not None:
            ok = False
        slot = getattr(p, "_rh_grad_slot", None)
        if slot is not None and len(slot) > 2 and slot[2] and not slot[1]:
            ok = False
        p._rh_pending = max(n - 1, 0)
        if p._rh_pending == 0:
            p._rh_shared = False
    return ok


class _OnSide:
    """``with _OnSide(device, tensors...)``: the body is enqueued on the side stream after everything already enqueued on
    the current stream; ``tensors`` are kept alive for it (caching-allocator stream bookkeeping)."""

    def __init__(self, device, *tensors, allow: bool = True, hold=()):
        """``hold``: gradient tensors RECEIVED from autograd that the body reads.  The same tensor object may sit in another
        node's input buffer (``y = conv(x) + other``: AddBackward hands ONE tensor to both branches), and autograd
        accumulates into a buffered gradient IN PLACE once it is the only holder -- on the compute stream, while the side
        stream still reads it.  A reference kept until the branch is joined makes that accumulation take the
        out-of-place form."""
        self.device = device
        self.tensors = [t for t in tensors if t is not None]
        self.hold = [t for t in hold if t is not None]
        self.active = allow and _side_enabled()

    def __enter__(self):
        if not self.active:
            return self
        self.main = torch.cuda.current_stream(self.device)
        self.side = SIDE.stream(self.device)
        self.side.wait_stream(self.main)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def keep(self, *tensors):
        self.tensors += [t for t in tensors if t is not None]

    def __exit__(self, *exc):
        if not self.active:
            return False
        self.ctx.__exit__(*exc)
        for t in self.tensors:
            t.record_stream(self.side)
        # The join is queued once per BACKWARD PASS (graph task).  A pass that raised after queueing never ran its callback
        # and left the pending state behind: a pending entry of ANOTHER pass is joined here and now, so that its
        # collected weight-norm launch still runs and a later pass queues its own join.
        task = _graph_task_id()
        if SIDE.pending is not None and SIDE.pending.task != task:
            SIDE.join()
        # (after the stale join, which clears SIDE.hold: this node's holds must survive until ITS join -- ADVICE r5)
        if _env("RH_SIDE_HOLD", "1") != "0":      # (0: the unprotected form, for the test that shows the race)
            SIDE.hold.extend(self.hold)
        if SIDE.pending is None:
            SIDE.pending = _Pending(self.main, self.side, task)
            try:        # end of this backward pass: the compute stream waits for the branch
                torch.autograd.Variable._execution_engine.queue_callback(SIDE.join)
            except RuntimeError:
                SIDE.join()       # not inside a backward pass (direct call): join at once
        return False
