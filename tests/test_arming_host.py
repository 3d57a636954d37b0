"""rave_amd._arming.armed_call, the one site that arms the thread-local state of the library, driven with a recording stand-in
for the library (no GPU): what it arms and in which order, and that everything armed is dropped when anything raises."""
import ctypes as C

import pytest


class _Lib:
    """Stand-in for ``_lib.lib``: the three arming functions and one entry point append to ``calls``."""

    def __init__(self, entry_raises=None, defer_raises=None):
        self.calls = []
        self.entry_raises, self.defer_raises = entry_raises, defer_raises

    def rh_x6_set_ranges(self, a, b, out, out2):
        self.calls.append(("set_ranges", a, b, out, out2))
        return 0

    def rh_defer_reduce(self, item):
        self.calls.append(("defer", item))
        if item is not None and self.defer_raises is not None:
            raise self.defer_raises
        return 0

    def rh_set_kernel_events(self, start, stop):
        self.calls.append(("events", start, stop))
        return 0

    def entry(self, rc):
        self.calls.append(("entry",))
        if self.entry_raises is not None:
            raise self.entry_raises
        return rc


class _Slot:
    """Stand-in for a slot tensor (``_lib.ptr`` takes its ``data_ptr()``)."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


DROPS = [("set_ranges", None, None, None, None), ("defer", None), ("events", None, None)]


@pytest.fixture
def arming(monkeypatch):
    from rave_amd import _arming

    def use(lib):
        monkeypatch.setattr(_arming.L, "lib", lib)
        return _arming
    return use


def test_arms_then_calls_and_passes_the_return_code_through(arming):
    lib = _Lib()
    A = arming(lib)
    assert A.armed_call(lambda: lib.entry(-7), in_b=_Slot(20), out=_Slot(30)) == -7
    assert lib.calls == [("set_ranges", None, 20, 30, None), ("entry",)]
    lib.calls.clear()
    item = A.L.ReduceItem()
    assert A.armed_call(lambda: lib.entry(0), in_a=_Slot(10), in_b=_Slot(20), out2=_Slot(40), defer=item, events=(1, 2)) == 0
    assert [c[0] for c in lib.calls] == ["events", "set_ranges", "defer", "entry"]
    assert lib.calls[0] == ("events", 1, 2) and lib.calls[1] == ("set_ranges", 10, 20, None, 40)
    assert C.addressof(lib.calls[2][1]._obj) == C.addressof(item)


def test_nothing_given_arms_nothing(arming):
    lib = _Lib()
    assert arming(lib).armed_call(lambda: lib.entry(3)) == 3
    assert lib.calls == [("entry",)]


def test_everything_is_dropped_when_the_entry_point_raises(arming):
    err = RuntimeError("injected")
    lib = _Lib(entry_raises=err)
    with pytest.raises(RuntimeError) as e:
        arming(lib).armed_call(lambda: lib.entry(0), in_b=_Slot(20), out=_Slot(30))
    assert e.value is err
    assert lib.calls == [("set_ranges", None, 20, 30, None), ("entry",)] + DROPS


def test_everything_is_dropped_when_arming_raises_part_way(arming):
    err = KeyboardInterrupt()
    lib = _Lib(defer_raises=err)
    A = arming(lib)
    with pytest.raises(KeyboardInterrupt) as e:
        A.armed_call(lambda: lib.entry(0), in_a=_Slot(10), defer=A.L.ReduceItem(), events=(1, 2))
    assert e.value is err
    assert [c[0] for c in lib.calls[:3]] == ["events", "set_ranges", "defer"]      # (the entry point was never reached)
    assert lib.calls[3:] == DROPS
