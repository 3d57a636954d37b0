"""Host side of the data feed's ``normalize`` / ``derivative`` steps (rave_amd/data.py, rh_feed_batch_post_i16_f32): the
numpy / scipy chain the GPU test compares with (tests/feed_chain.py) against the unmodified reference where it is present,
the constructor's arguments, the entry point's refusals (host checks, nothing is launched) and the test inputs themselves."""
import ctypes as C
import importlib
import inspect
import sys
import types

import numpy as np
import pytest
import torch

import feed_chain as F


@pytest.fixture(scope="module")
def pcm():
    return F.make_pcm()


@pytest.fixture(scope="module")
def noise():
    return F.make_noise()


@pytest.fixture(scope="module")
def items64(pcm, noise):
    """The six items behind Dequantize in float64, all-pass on for items 0, 2, 4."""
    return F.dequantized(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES, variant="ref64")


@pytest.fixture
def reference_dataset(monkeypatch):
    """The unmodified rave/dataset.py.  Its imports name ``udls`` (the lmdb container classes), which neither this machine
    nor oracle/shims has; the two functions under test touch none of it, so empty stand-ins are registered for the length of
    the test, and the modules imported under them are dropped again."""
    from ref_import import import_reference, reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    import_reference()
    before = set(sys.modules)
    for name, attrs in (("udls", ("AudioExample",)), ("udls.transforms", ()), ("udls.generated", ("AudioExample",))):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, type(a, (), {}))
            monkeypatch.setitem(sys.modules, name, mod)
    import lmdb                                                   # oracle/shims: only what rave/__init__ needs
    if not hasattr(lmdb, "Environment"):
        monkeypatch.setattr(lmdb, "Environment", type("Environment", (), {}), raising=False)
    try:
        yield importlib.import_module("rave.dataset")
    except (ImportError, AttributeError) as e:
        pytest.skip(f"rave.dataset cannot be imported here: {e}")
    finally:
        for name in set(sys.modules) - before:
            if name.startswith("rave."):
                sys.modules.pop(name)


def test_helper_equals_the_reference_functions(items64, reference_dataset):
    dataset = reference_dataset
    derive = dataset.get_derivator_integrator(44100)[0]
    for b, x in enumerate(items64):
        for cap in (30, 12.5, 0):
            want = dataset.normalize_signal(x.copy(), cap)
            got = F.normalize_signal(x.copy(), cap)
            assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), (b, cap)
        want = derive(x.copy())
        assert want.dtype == np.float64 and np.array_equal(F.derivator(x.copy()), want), b
        assert np.array_equal(F.derivator(F.normalize_signal(x.copy())), derive(dataset.normalize_signal(x.copy()))), b
    # the float32 items of the ``ref32`` variant (an unfiltered item stays float32 through normalize_signal)
    x32 = items64[F.QUIET].astype(np.float32)
    want = dataset.normalize_signal(x32.copy())
    got = F.normalize_signal(x32.copy())
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_flags_default_off_and_a_bad_max_gain_db_raises():
    from rave_amd import data as D
    sig = inspect.signature(D.GpuBatchFeed.__init__).parameters
    assert sig["normalize"].default is False and sig["derivative"].default is False and sig["max_gain_db"].default == 30.
    assert D.check_max_gain_db(12) == 12.0 and isinstance(D.check_max_gain_db(np.float32(6)), float)
    host = torch.zeros(1, 1, 8, dtype=torch.int16)
    for bad in (float("nan"), float("inf"), -float("inf"), None, "30", True):
        with pytest.raises(RuntimeError, match="max_gain_db"):
            D.check_max_gain_db(bad)
        with pytest.raises(RuntimeError, match="max_gain_db"):           # refused before anything else is looked at
            D.GpuBatchFeed(host, normalize=True, max_gain_db=bad)


def test_inputs_exercise_the_branches(items64):
    peaks = [float(np.abs(x).max()) for x in items64]
    # the quiet item is beyond the cap: exactly 10^(30 / 20)
    assert peaks[F.QUIET] < 10 ** -1.5
    assert F.gain_of(peaks[F.QUIET]) == 10 ** 1.5
    assert np.array_equal(F.normalize_signal(items64[F.QUIET]), items64[F.QUIET] * 10 ** 1.5)
    # the full-scale item is attenuated (its peak is above 1: -32768 / 32767, the all-pass and the noise on top), to peak 1
    g = F.gain_of(peaks[F.FULL])
    assert peaks[F.FULL] > 1 and g < 1 and abs(g * peaks[F.FULL] - 1) < 1e-12
    # the stereo item's peak is not in its first row, and a per-row peak would give row 0 another gain
    row_peaks = np.abs(items64[F.LOUD1]).max(-1)
    assert row_peaks[1] == peaks[F.LOUD1] and row_peaks[0] < row_peaks[1] / 10
    assert F.gain_of(row_peaks[0]) > 4 * F.gain_of(row_peaks[1])
    # the all-zero item is zero only when the noise is
    zero = F.dequantized(F.make_pcm(), np.zeros_like(F.make_noise()), F.ITEMS, F.IN_POINTS, F.ANGLES_FLIPPED)[F.ZERO]
    assert not zero.any() and F.gain_of(0.0) == 1.0 and not F.normalize_signal(zero).any()
    # ordinary items: a gain above 1, below the cap
    for b in (4, 5):
        assert 1 < F.gain_of(peaks[b]) < 10 ** 1.5


def test_variants_hold_the_dtypes_they_claim(pcm, noise):
    r32 = F.dequantized(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES, variant="ref32")
    for b, x in enumerate(r32):
        assert x.dtype == (np.float32 if F.ANGLES[b] is None else np.float64)
        assert F.normalize_signal(x).dtype == x.dtype and F.derivator(x).dtype == np.float64
    kw = dict(normalize=True, derivative=True)
    a = F.chain(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES, variant="ref32", **kw)
    b = F.chain(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES, variant="ref64", **kw)
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == (F.N_ITEMS, F.CH, F.N)
    for i in range(F.N_ITEMS):
        for c in range(F.CH):
            assert np.abs(a[i, c] - b[i, c]).max() <= 4 * 2.0 ** -24 * max(np.abs(b[i]).max(), 2.0 ** -16)


def _table(n_rows, length):
    from rave_amd import data as D
    t = np.zeros(n_rows, dtype=D.ROW_DTYPE)
    t["coef"] = np.nan
    t["length"] = length
    t["up"] = t["down"] = 1
    t["base"] = np.arange(n_rows) * length
    return t


def test_entry_point_refuses_on_the_host_table_without_a_launch():
    """No GPU here: a call that got as far as a launch would fail with another message than the ones matched below."""
    from rave_amd import _lib as L
    n_rows, length, n = 4, 64, 48
    t = _table(n_rows, length)
    need = L.lib.rh_feed_post_workspace_bytes(n_rows, n)
    assert need == (n_rows * n + n_rows) * 8 and L.lib.rh_feed_post_workspace_bytes(0, n) == 0
    assert L.lib.rh_feed_post_workspace_bytes(-1, n) < 0 and L.lib.rh_feed_post_workspace_bytes(1, 0) < 0
    buf = (C.c_double * (need // 8 + 2))()
    a = C.addressof(buf)

    def call(rows=n_rows, n_ch=2, norm=1, cap=30.0, der=1, ws=a, ws_bytes=need, table=t):
        return L.lib.rh_feed_batch_post_i16_f32(a, n_rows * length, table.ctypes.data, a, None, 0, a, rows, n, 16, n_ch, norm, cap,
                                                der, ws, ws_bytes, a, None)

    for kw, word in ((dict(rows=3), b"whole items"), (dict(n_ch=0), b"whole items"), (dict(n_ch=3), b"whole items"),
                     (dict(cap=float("nan")), b"max_gain_db"), (dict(cap=float("inf")), b"max_gain_db"),
                     (dict(ws_bytes=need - 8), b"workspace"), (dict(ws=None), b"workspace"), (dict(ws=a + 4), b"8-byte")):
        assert call(**kw) != 0 and word in L.lib.rh_last_error(), (kw, L.lib.rh_last_error())
    assert call(cap=float("nan"), norm=0, der=0) != 0 and b"max_gain_db" in L.lib.rh_last_error()     # also with both steps off
    bad = t.copy()
    bad["in_point"][3] = length - n + 1                                                              # the pitched entry point's checks
    assert call(table=bad) != 0 and b"row 3" in L.lib.rh_last_error()
    bad = t.copy()
    bad["up"][1] = 20
    assert call(table=bad) != 0 and b"row 1" in L.lib.rh_last_error()
    assert call(rows=0, ws=None, ws_bytes=0) == 0                                                    # no rows: nothing to do


class _HostPcm:
    """Stand-in for the resident PCM (as in tests/test_feed_resample_host.py): a feed looks at its type, shape and device."""
    dtype, is_cuda, device = torch.int16, True, torch.device("cpu")

    def __init__(self, n_ch):
        self.shape = (F.N_ITEMS, n_ch, F.LENGTH)

    def dim(self):
        return 3

    def contiguous(self):
        return self


def _loop_table(D, feed, n_ch, items, in_points, angles, ratios, mute):
    """The row table as ``GpuBatchFeed.sample`` filled it before ``_row_table``: row by row, field by field."""
    batch, length = len(items), F.LENGTH
    table = np.zeros(batch * n_ch, dtype=D.ROW_DTYPE)
    table["coef"] = np.nan
    table["length"] = length
    table["up"] = table["down"] = 1
    for b in range(batch):
        ratio = ratios[b] if ratios is not None else None
        for c in range(n_ch):
            row = table[b * n_ch + c]
            row["base"] = (int(items[b]) * n_ch + c) * length
            row["in_point"] = int(in_points[b])
            row["mute"] = int(mute is not None and bool(mute[b]))
            if angles[b] is not None:
                bb, aa = D.pole_to_z_filter(angles[b], .99)
                row["coef"] = [bb[0], bb[1], bb[2], aa[1], aa[2]]
            if ratio is not None:
                row["up"], row["down"] = int(ratio[0]), int(ratio[1])
                row["mean"] = feed.means[int(items[b]) * n_ch + c]
                row["tap_offset"] = feed._tap_offset(ratio)
    return table


def _loop_plain(D, n_ch, items, in_points, angles):
    """``src_offset`` and ``coef`` of the plain launch as ``sample`` filled them in a loop of their own."""
    batch, length = len(items), F.LENGTH
    off = np.empty(batch * n_ch, dtype=np.int64)
    coef = np.full((batch * n_ch, 5), np.nan, dtype=np.float64)
    for b in range(batch):
        for c in range(n_ch):
            r = b * n_ch + c
            off[r] = (int(items[b]) * n_ch + c) * length + int(in_points[b])
            if angles[b] is not None:
                bb, aa = D.pole_to_z_filter(angles[b], .99)
                coef[r] = [bb[0], bb[1], bb[2], aa[1], aa[2]]
    return off, coef


@pytest.mark.parametrize("n_ch", [1, 2])
@pytest.mark.parametrize("with_table", [True, False], ids=["rand_pitch", "no-rand_pitch"])
def test_row_table_is_the_loop_it_replaces_byte_for_byte(n_ch, with_table):
    from rave_amd import data as D
    feed = D.GpuBatchFeed(_HostPcm(n_ch))
    if with_table:
        feed.pitch = D.PitchTable(F.PITCH_RANGE)
    feed.means = np.random.default_rng(11).standard_normal(F.N_ITEMS * n_ch)      # what ``_means`` returns once it is cached
    mute = np.array([False, True, True, False, False, True])
    # (1, 19) and (0, 5) are outside every table: sentinel -1; (3, 3) reduces to 1/1: sentinel 0 with a table, -1 without
    odd = [(13, 10), (1, 19), (3, 3), None, (0, 5), (14, 19)]
    for ratios in (None, [None] * F.N_ITEMS, F.RATIOS, odd):
        for m in (None, mute, list(mute), [False] * F.N_ITEMS):
            for items, in_points, angles in ((F.ITEMS, F.IN_POINTS, F.ANGLES), (F.ITEMS[::-1], F.PITCH_IN_POINTS, F.ANGLES_FLIPPED),
                                             (list(F.ITEMS), list(F.IN_POINTS), [None] * F.N_ITEMS)):
                got = feed._row_table(items, in_points, angles, ratios, m)
                want = _loop_table(D, feed, n_ch, items, in_points, angles, ratios, m)
                assert got.dtype == want.dtype == D.ROW_DTYPE and got.shape == want.shape == (F.N_ITEMS * n_ch,)
                assert got.tobytes() == want.tobytes(), (ratios, m, angles)
                off, coef = _loop_plain(D, n_ch, items, in_points, angles)
                src_offset, table_coef = got["base"] + got["in_point"], np.ascontiguousarray(got["coef"])
                assert src_offset.dtype == off.dtype and src_offset.tobytes() == off.tobytes()
                assert table_coef.dtype == coef.dtype and table_coef.shape == coef.shape and table_coef.tobytes() == coef.tobytes()
    taps = feed._row_table(F.ITEMS, F.PITCH_IN_POINTS, F.ANGLES, odd, None)["tap_offset"][::n_ch]
    assert list(taps[[1, 2, 3, 4]]) == ([-1, 0, 0, -1] if with_table else [-1, -1, 0, -1])
    assert (taps[0] >= 0 and taps[5] > 0 and taps[0] != taps[5]) if with_table else (taps[0] == taps[5] == -1)
