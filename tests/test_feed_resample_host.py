"""Host side of the data feed's ``resample_to`` option (rave_amd/data.py, rh_feed_batch_resample_i16_f32): torchaudio's filter
table and output length against the model (tests/resample_reference.py) and against figures worked out from the formula, the
envelope of rates, the arithmetic the kernel is specified to use against the bar of the GPU test, the draws, the length rule of
``freq_mask`` and the entry point's refusals (host checks, nothing is launched)."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest
import torch

import feed_chain as F
import resample_reference as R


class HostPcm:
    """Stand-in for the resident PCM, so that a feed can be built without a GPU (as in tests/test_feed_mask_host.py): the
    constructor and ``draw`` look at nothing but its type, its shape and its device."""
    dtype, is_cuda, device = torch.int16, True, torch.device("cpu")

    def __init__(self, n_items=64, n_ch=2, length=20000):
        self.shape = (n_items, n_ch, length)

    def dim(self):
        return 3

    def contiguous(self):
        return self


def _table(n_rows, length):
    from rave_amd import data as D
    t = np.zeros(n_rows, dtype=D.ROW_DTYPE)
    t["coef"] = np.nan
    t["length"] = length
    t["up"] = t["down"] = 1
    t["base"] = np.arange(n_rows) * length
    return t


@pytest.mark.parametrize("rates", list(R.RATIOS) + [(88200, 32000)], ids=lambda r: f"{r[0]}-{r[1]}")
def test_table_is_the_models_bit_for_bit(rates):
    from rave_amd import data as D
    table, width = D.sinc_resample_kernel(*rates)
    want, want_width = R.sinc_kernel(*rates, torch.float32)
    (o, n), (w, k) = R.RATIOS[rates][:2] if rates in R.RATIOS else ((441, 160), (17, 475))
    assert (width, want_width) == (w, w) and table.shape == want.shape == (n, k) and k == 2 * w + o
    assert table.dtype == torch.float32 and table.device.type == "cpu" and torch.equal(table, want)
    # a low-pass of unit gain at DC: the n filters sum to ~n; and the float64 table is the same function (the float32 one
    # takes sin and cos of float32 arguments of up to 6 pi, rounded several times on the way: a few 1e-6 each, taps <= 1)
    assert abs(float(table.double().sum()) / n - 1) < 1e-2
    assert float((table.double() - R.sinc_kernel(*rates, torch.float64)[0]).abs().max()) < 1e-4


def test_lengths():
    from rave_amd import data as D
    for rates, (_, _, n_res) in R.RATIOS.items():
        assert D.sinc_resampled_length(F.N, *rates) == R.resampled_length(F.N, *rates) == n_res, rates
    assert D.sinc_resampled_length(100, 48000, 44100) == 92
    assert D.sinc_resampled_length(65536, 88200, 44100) == 32768 and D.sinc_resampled_length(8192, 88200, 44100) == 4096
    assert D.sinc_resampled_length(F.N, 44100, 44100) == F.N


def _call(L, n_rows=4, n=48, length=64, n_ch=2, norm=1, cap=30.0, der=1, orig=48000, new=44100, res_taps=True, n_res_taps=None,
          width=None, ws=True, ws_bytes=None, ws_offset=0, table=None):
    """The entry point on host buffers: with every argument in order it would reach the launch, which no test here lets it."""
    o, nn = R.reduced(orig, new) if min(orig, new) >= 1 else (1, 1)
    w = int(np.ceil(6.0 * o / (min(o, nn) * 0.99)))
    need = max(L.lib.rh_feed_resample_workspace_bytes(n_rows, n, orig, new), 8)
    buf = (C.c_double * (need // 8 + 2))()
    a = C.addressof(buf)
    t = _table(n_rows, length) if table is None else table
    return L.lib.rh_feed_batch_resample_i16_f32(a, n_rows * length, t.ctypes.data, a, None, 0, a, n_rows, n, 16, n_ch, norm, cap, der,
                                                orig, new, a if res_taps else None, nn * (2 * w + o) if n_res_taps is None else n_res_taps,
                                                w if width is None else width, a + ws_offset if ws else None,
                                                need if ws_bytes is None else ws_bytes, a, None)


def test_every_pair_of_the_envelope_is_accepted():
    from rave_amd import _lib as L, data as D
    worst_k, worst_table = (0, None), (0, None)
    for orig, new in itertools.permutations(R.ENVELOPE, 2):
        o, n = R.reduced(orig, new)
        width = int(np.ceil(6 * o / (min(o, n) * 0.99)))
        k = 2 * width + o
        assert k <= D.RES_SPAN and n <= D.RES_OUT, (orig, new)
        worst_k, worst_table = max(worst_k, (k, (orig, new))), max(worst_table, (4 * n * k, (orig, new)))
        # the entry point gets past the table and the envelope and stops at the workspace
        assert _call(L, orig=orig, new=new, ws=False) != 0 and b"workspace" in L.lib.rh_last_error(), (orig, new, L.lib.rh_last_error())
    # 96000 -> 22050 is 640/147: width 27; 22050 -> 32000 is 441/640: 640 filters of 455 taps, 1.16 MB
    assert worst_k == (694, (96000, 22050)) and worst_table == (4 * 640 * 455, (22050, 32000))
    for orig, new in ((96000, 22050), (22050, 32000), (16000, 96000)):      # the tables themselves, where they are largest
        table, width = D.check_resample(orig, new)
        o, n = R.reduced(orig, new)
        assert table.shape == (n, 2 * width + o) and bool(torch.isfinite(table).all())


def test_rates_outside_the_kernels_constants_are_refused_by_name():
    from rave_amd import _lib as L, data as D
    pcm = HostPcm()
    for (orig, new), word in (((8209, 1), "kResSpan"), ((1, 6151), "kResOut")):
        with pytest.raises(RuntimeError, match=word):
            D.check_resample(orig, new)
        with pytest.raises(RuntimeError, match=word):
            D.GpuBatchFeed(pcm, sr=orig, resample_to=new)
        assert _call(L, orig=orig, new=new) != 0 and word.encode() in L.lib.rh_last_error(), L.lib.rh_last_error()
    for bad in (0, -44100, 44100.0, "44100", True):
        with pytest.raises(RuntimeError, match="Resample"):
            D.GpuBatchFeed(pcm, sr=48000, resample_to=bad)


def test_entry_point_refuses_on_the_host_without_a_launch():
    """No GPU here: a call that got as far as a launch would fail with another message than the ones matched below."""
    from rave_amd import _lib as L
    n_rows, n = 4, 48
    n_res = R.resampled_length(n, 48000, 44100)
    need = L.lib.rh_feed_resample_workspace_bytes(n_rows, n, 48000, 44100)
    assert n_res == 45 and need == ((n_rows * n + n_rows) + (n_rows * n_res + n_rows)) * 8
    assert L.lib.rh_feed_resample_workspace_bytes(n_rows, n, 44100, 44100) == L.lib.rh_feed_post_workspace_bytes(n_rows, n)
    assert L.lib.rh_feed_resample_workspace_bytes(0, n, 48000, 44100) == 0
    for bad in ((-1, n, 48000, 44100), (1, 0, 48000, 44100), (1, n, 0, 44100), (1, n, 48000, -1), (1, 2 ** 31 - 1, 1, 2)):
        assert L.lib.rh_feed_resample_workspace_bytes(*bad) < 0, bad
    for kw, word in ((dict(n_rows=3), b"whole items"), (dict(n_ch=0), b"whole items"), (dict(n_ch=3), b"whole items"),
                     (dict(cap=float("nan")), b"max_gain_db"), (dict(cap=float("inf")), b"max_gain_db"),
                     (dict(orig=0), b"rates"), (dict(new=-1), b"rates"),
                     (dict(width=6), b"width"), (dict(width=8), b"width"), (dict(n_res_taps=147 * 174 - 1), b"taps"),
                     (dict(n_res_taps=147 * 174 + 1), b"taps"), (dict(n_res_taps=174), b"taps"), (dict(res_taps=False), b"null"),
                     (dict(ws_bytes=need - 8), b"workspace"), (dict(ws=False), b"workspace"), (dict(ws_offset=4), b"8-byte"),
                     (dict(n=2 ** 31 - 1, orig=22050, new=44100, length=2 ** 31 - 1, n_rows=2), b"int32")):
        assert _call(L, **kw) != 0 and word in L.lib.rh_last_error(), (kw, L.lib.rh_last_error())
    bad = _table(n_rows, 64)                                  # the pitched entry point's checks on the row table
    bad["in_point"][3] = 64 - n + 1
    assert _call(L, table=bad) != 0 and b"row 3" in L.lib.rh_last_error()
    bad = _table(n_rows, 64)
    bad["up"][1] = 20
    assert _call(L, table=bad) != 0 and b"row 1" in L.lib.rh_last_error()
    assert _call(L, n_rows=0, ws=False, ws_bytes=0) == 0      # no rows: nothing to do
    # equal rates are the post entry point, whatever the table arguments say: its refusals, under its name
    assert _call(L, orig=44100, new=44100, width=-5, n_res_taps=3, ws=False) != 0 and b"feed_batch_post: workspace" in L.lib.rh_last_error()


def test_a_feed_with_resample_draws_as_one_without():
    from rave_amd import data as D
    sig = inspect.signature(D.GpuBatchFeed.__init__).parameters
    assert sig["resample_to"].default is None
    pcm = HostPcm()
    feeds = [D.GpuBatchFeed(pcm, sr=48000, seed=5), D.GpuBatchFeed(pcm, sr=48000, seed=5, resample_to=None),
             D.GpuBatchFeed(pcm, sr=48000, seed=5, resample_to=48000), D.GpuBatchFeed(pcm, sr=48000, seed=5, resample_to=44100)]
    assert [f.resample_to for f in feeds] == [None, None, None, 44100] and feeds[2].res_taps is None
    assert feeds[3].res_taps.shape == (147, 174) and feeds[3].res_taps.dtype == torch.float32 and feeds[3].res_width == 7
    for _ in range(3):
        draws = [f.draw(16, 8192) for f in feeds]
        for d in draws[1:]:
            assert len(d) == len(draws[0]) == 3
            assert np.array_equal(d[0], draws[0][0]) and np.array_equal(d[1], draws[0][1]) and d[2] == draws[0][2]
    rng = np.random.default_rng(5)
    for _ in range(3):
        D.draw_batch(rng, 64, 20000, 16, 8192, 48000, .8, None)
    assert feeds[0].rng.random() == feeds[3].rng.random() == rng.random()
    # the dequantisation noise is drawn for the n_signal samples in front of Resample: the device generators stay in step too
    a, b = (torch.rand(32, 8192, device=f.gen.device, generator=f.gen) for f in (feeds[0], feeds[3]))
    assert torch.equal(a, b)


def test_freq_mask_length_rule_applies_to_the_resampled_length():
    from rave_amd import data as D
    pcm = HostPcm()
    feed = D.GpuBatchFeed(pcm, sr=88200, resample_to=44100, freq_mask=.5)
    for n in (4096, 6144, 8190, 12290):                     # 2048, 3072, 4095, 6145 resampled samples
        with pytest.raises(RuntimeError, match="multiple of 2048"):
            feed.sample(4, n)
    # 8192 -> 4096 passes the rule (and then needs the GPU); without Resample the same feed refuses 6144 and takes 8192
    plain = D.GpuBatchFeed(pcm, sr=88200, freq_mask=.5)
    with pytest.raises(RuntimeError, match="multiple of 2048"):
        plain.sample(4, 6144 + 1024)
    up = D.GpuBatchFeed(pcm, sr=22050, resample_to=44100, freq_mask=.5)
    with pytest.raises(RuntimeError, match="multiple of 2048"):
        up.sample(4, 1024)                                  # 2048 resampled samples: below two hops
    with pytest.raises(RuntimeError, match="multiple of 2048"):
        up.sample(4, 2048 + 512)                            # 5120


@pytest.mark.parametrize("amplitude", [1.0, 0.003], ids=["full-scale", "quiet"])
@pytest.mark.parametrize("rates,n", [(r, F.N) for r in R.RATIOS] + [((48000, 44100), 160), ((48000, 44100), 100)],
                         ids=lambda v: f"{v[0]}-{v[1]}" if isinstance(v, tuple) else str(v))
def test_specified_arithmetic_is_inside_the_bar(rates, n, amplitude):
    """float32 taps times float32 samples, summed in float64 and rounded once -- what the kernel is specified to do -- against
    the bar of the GPU test, 2 max |ref32 - ref64| + 2^-23 max |ref64| per row, on the model alone: a bar the specified
    arithmetic itself missed could not be held by any kernel.  The ratio is printed: about one half, the factor 2 is margin."""
    rng = np.random.default_rng(3)
    x = amplitude * rng.uniform(-1, 1, (F.CH, n))
    ref32, ref64, got = R.resample(x, *rates, "ref32"), R.resample(x, *rates, "ref64"), R.kernel_arithmetic(x, *rates)
    assert ref32.dtype == got.dtype == np.float32 and ref64.dtype == np.float64
    assert ref32.shape == ref64.shape == got.shape == (F.CH, R.resampled_length(n, *rates))
    for c in range(F.CH):
        err, bound = float(np.abs(got[c] - ref64[c]).max()), F.row_bound(ref32[c], ref64[c])
        print(f"{rates} n = {n} amplitude {amplitude}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
        assert err <= bound, (c, err, bound)
