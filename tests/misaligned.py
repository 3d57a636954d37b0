"""Tensors at pointers that are only 4-byte aligned, with guard bands around them (a plain helper module, no fixtures).

include/rave_hip.h asks for "contiguous fp32, every pointer a device pointer owned by the caller" and nowhere for 16-byte
alignment, while every tensor of torch's caching allocator is 512-byte aligned.  ``carve`` places a copy of a tensor at a chosen
residue of its address modulo 16 inside a larger buffer whose every other element holds a guard pattern (a quiet NaN for the
floating-point types: a kernel that READS a guard poisons its output); ``guards_intact`` then tells, bit for bit, whether a
kernel WROTE outside the tensor.  ``BucketReducer`` is rave_amd.ddp.GradReducer for ONE process without a process group:
gradients are written into, and adopted from, the views of the flat bucket exactly as under data parallelism; only the
collective itself is left out.
"""
import weakref

import torch

from test_gpu_wgrad_wide import _Env  # noqa: F401  (re-exported: the tests that use this module set kernel switches with it)

# guard patterns, as the integer type of the same width: quiet NaNs for float / double, a value no test produces for integers
_GUARD = {
    torch.float32: (torch.int32, 0x7FC00000),
    torch.float64: (torch.int64, 0x7FF8000000000000),
    torch.int16: (torch.int16, -0x3F40),
    torch.int32: (torch.int32, 0x7FC00000),
    torch.int64: (torch.int64, 0x7FF8000000000000),
}


# data_ptr -> the view carve() returned, while that view is alive: lets guards_intact() take any tensor that starts at the same
# address (a .detach(), a .view(), the .data of a Parameter made from the view), which does not carry the view's attribute
_VIEWS = weakref.WeakValueDictionary()


def _record(t):
    rec = getattr(t, "_carved", None)
    if rec is None:
        rec = _VIEWS[t.data_ptr()]._carved
    return rec


def carve(t, off, guard=64):
    """A contiguous copy of ``t`` (host or device) whose ``data_ptr() % 16 == 4 * off`` (``off`` in 0..3), in the middle of a
    fresh flat buffer with at least ``guard`` guard elements on either side.  Types wider than 4 bytes can only take the
    residues that are multiples of their size (int64 / double: off 0 and 2)."""
    assert 0 <= off <= 3
    ity, pat = _GUARD[t.dtype]
    es = t.element_size()
    n = t.numel()
    buf = torch.empty(n + 2 * guard + 16, dtype=t.dtype, device=t.device)
    buf.view(ity).fill_(pat)
    need = (4 * off - buf.data_ptr()) % 16          # bytes from the buffer's start to the first address of that residue
    assert need % es == 0, f"a {t.dtype} tensor cannot start at byte residue {4 * off}"
    start = need // es
    while start < guard:
        start += 16 // es
    view = buf[start:start + n]
    view.copy_(t.detach().reshape(-1))
    view = view.view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off, (view.data_ptr() % 16, off)
    assert start >= guard and buf.numel() - (start + n) >= guard
    view._carved = (buf, start, n)
    _VIEWS[view.data_ptr()] = view
    return view


def guards_intact(view):
    """True iff every element of the carved buffer outside ``view`` still holds the guard pattern (compared as integers: a NaN
    never equals itself)."""
    buf, start, n = _record(view)
    ity, pat = _GUARD[buf.dtype]
    bits = buf.view(ity)
    return bool((bits[:start] == pat).all()) and bool((bits[start + n:] == pat).all())


def fill_guard(t):
    """Overwrites a tensor of any type carve() knows with its guard pattern, in place (for slots that nothing may write)."""
    ity, pat = _GUARD[t.dtype]
    t.view(ity).fill_(pat)


def is_guard(t):
    ity, pat = _GUARD[t.dtype]
    return bool((t.view(ity) == pat).all())


def residues(reducer):
    """Histogram {storage_offset % 4: count} over the gradient views of a GradReducer (the flat buffers themselves are 16-byte
    aligned, so this is the views' address residue in floats)."""
    hist = {0: 0, 1: 0, 2: 0, 3: 0}
    for b in reducer.buckets:
        assert b.flat.data_ptr() % 16 == 0
        for v in b.views:
            hist[v.storage_offset() % 4] += 1
    return hist


def bucket_reducer(params, **kw):
    """rave_amd.ddp.GradReducer over ``params`` in ONE process without a process group.  The reducer is forced on (with
    ``world == 1`` it is otherwise disabled and no view is handed out), and the bucket's departure does everything the real one
    does -- the collected weight-norm backward and deferred reductions of the side stream are flushed -- except the
    all-reduce, which needs a process group and changes nothing for a single rank."""
    from rave_amd import ddp, ops

    class BucketReducer(ddp.GradReducer):
        def _launch(self, b):
            if b.flat.is_cuda:
                ops.side_stream_for_collective(b.flat.device)
            b.launched = True

    return BucketReducer(params, force=True, **kw)
