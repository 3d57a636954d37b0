"""The one place that arms the thread-local state of the library (include/rave_hip.h).

Three calls arm state that the NEXT entry point of the calling thread consumes: rh_x6_set_ranges (the range slots of the f16
matrix-core kernels), rh_defer_reduce (a weight gradient leaves its K-slice partials to the caller) and rh_set_kernel_events
(the next main kernel is dispatched between two HIP events).  Whatever is armed and not consumed -- anything raised between the
arming and the entry point, the entry point itself included -- would reach the next, unrelated call of the thread: every arming
site therefore goes through ``armed_call``, which drops all three before it re-raises.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L


def drop() -> None:
    """Drop whatever the three arming calls left for the next call of this thread."""
    lib = L.lib
    lib.rh_x6_set_ranges(None, None, None, None)
    lib.rh_defer_reduce(None)
    lib.rh_set_kernel_events(None, None)


def armed_call(call, in_a=None, in_b=None, out=None, out2=None, defer=None, events=None):
    """Arm what is given -- ``in_a`` / ``in_b`` / ``out`` / ``out2``: range slots (tensors), ``defer``: a ReduceItem, ``events``: a
    (start, stop) pair of HIP event handles --, make ``call()`` (the entry point that consumes it) and return its return code.
    Nothing given: nothing is armed (the bf16 build arms nothing).  Calls nest: ``call`` may itself arm more on its way to the
    entry point (the profiled launch arms the events around a launch that arms its slots)."""
    lib = L.lib
    try:
        if events is not None:
            lib.rh_set_kernel_events(*events)
        if in_a is not None or in_b is not None or out is not None or out2 is not None:
            lib.rh_x6_set_ranges(L.ptr(in_a), L.ptr(in_b), L.ptr(out), L.ptr(out2))
        if defer is not None:
            lib.rh_defer_reduce(C.byref(defer))
        return call()
    except BaseException:
        drop()
        raise
