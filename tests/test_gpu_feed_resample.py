"""``GpuBatchFeed(resample_to=...)`` (rh_feed_batch_resample_i16_f32, rave_amd/data.py) against the reference's chain with
``transforms.Resample`` behind Dequantize, restated with torch CPU ops and numpy / scipy (tests/resample_reference.py,
tests/feed_chain.py) on injected draws: 6 stereo items x 6000 samples, batch 6, n_signal = 4352 = one full 4096-sample chunk of
the chain kernel plus a ragged one.  At 48000 -> 44100 (160/147, 174 taps) that is 3999 = 27 * 147 + 30 outputs, 28 frames of
which the last is cut: one pass of the resampling kernel (41 frames at this ratio); 22050 -> 44100 takes two passes at this
length, and test_rows_longer_than_one_pass three with a partial last one at 160/147.  The one bar, per row
(tests/test_gpu_feed_pitch.py):
    max |got - ref64| <= 2 max |ref32 - ref64| + 2^-23 max |ref64|
measured on the model alone; the arithmetic the kernel is specified to use stays at about half of it
(tests/test_feed_resample_host.py)."""
import functools

import numpy as np
import pytest
import torch

import feed_chain as F
import resample_reference as R

pytestmark = pytest.mark.gpu

B, CH, N = F.N_ITEMS, F.CH, F.N
FLAGS = {"none": {}, "normalize": dict(normalize=True), "derivative": dict(derivative=True),
         "both": dict(normalize=True, derivative=True)}
MAIN = (48000, 44100)
CASES = [(MAIN, k, N) for k in FLAGS] + [(r, k, N) for r in R.RATIOS if r != MAIN for k in ("none", "both")] \
    + [(MAIN, "none", 100), (MAIN, "both", 100)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pcm_d(dev):
    return torch.from_numpy(F.make_pcm()).to(dev)


@functools.lru_cache(maxsize=None)
def noise(n=N):
    return np.ascontiguousarray(F.make_noise()[:, :n])


@functools.lru_cache(maxsize=None)
def reference(rates, flags, n=N, in_points=tuple(F.IN_POINTS), ratios=None, mute=None, items=tuple(F.ITEMS), angles=tuple(F.ANGLES)):
    """(ref32, ref64) of one case, computed once."""
    return tuple(R.chain(F.make_pcm(), noise(n)[:CH * len(items)], list(items), list(in_points), list(angles), *rates,
                         ratios=None if ratios is None else list(ratios), mute=mute, variant=v, n=n, **FLAGS[flags])
                 for v in ("ref32", "ref64"))


@functools.lru_cache(maxsize=None)
def feed_of(pcm_d, rates, flags, **kw):
    from rave_amd import data as D
    return D.GpuBatchFeed(pcm_d, sr=rates[0], seed=1, resample_to=rates[1], **FLAGS[flags], **kw)


def run(feed, n=N, in_points=F.IN_POINTS, ratios=None, mute=None, items=F.ITEMS, angles=F.ANGLES, bands=None):
    draws = (items, in_points, angles) if ratios is None else (items, in_points, angles, ratios)
    nz = torch.from_numpy(noise(n)[:CH * len(items)])
    y = feed.sample(len(items), n, draws=draws, noise=nz, mute=mute, bands=bands)
    n_res = n if feed.resample_to is None else R.resampled_length(n, feed.sr, feed.resample_to)
    assert y.shape == (len(items), CH, n_res) and y.dtype == torch.float32 and y.is_contiguous()
    return y


def check_rows(got, ref32, ref64, what):
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape)
    for b in range(got.shape[0]):
        for c in range(CH):
            err = float(np.abs(got[b, c].astype(np.float64) - ref64[b, c]).max())
            bound = F.row_bound(ref32[b, c], ref64[b, c])
            print(f"{what} row {b}.{c}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f} (max |ref| {np.abs(ref64[b, c]).max():.3e})")
            assert np.isfinite(got[b, c]).all() and err <= bound, (what, b, c, err, bound)


@pytest.mark.parametrize("rates,flags,n", CASES, ids=[f"{r[0]}-{r[1]}-{k}-{n}" for r, k, n in CASES])
def test_resampled_feed_matches_the_reference_chain(pcm_d, rates, flags, n):
    y = run(feed_of(pcm_d, rates, flags), n).cpu().numpy()
    ref32, ref64 = reference(rates, flags, n)
    if n == N:
        assert y.shape[-1] == R.RATIOS[rates][2]
    check_rows(y, ref32, ref64, f"{rates} {flags} n = {n}")


@pytest.mark.parametrize("flags", ["none", "both"])
def test_both_zero_padded_ends_carry_full_scale_data(pcm_d, flags):
    """The full-scale item cropped at its first and at its last sample: the `width` zeros in front of the row, the
    `width + o` behind it and the cut last frame (3999 = 27 * 147 + 30) all sit under taps that meet samples of order 1."""
    items, in_points, angles = (F.FULL, F.FULL), (0, F.LENGTH - N), (None, 0.05)
    kw = dict(items=items, in_points=in_points, angles=angles)
    y = run(feed_of(pcm_d, MAIN, flags), **kw).cpu().numpy()
    ref32, ref64 = reference(MAIN, flags, **kw)
    assert y.shape[-1] == 3999 == 27 * 147 + 30
    plain = reference(MAIN, "none", **kw)[1]
    assert (np.abs(plain[..., :4]).max(-1) > .05).all() and (np.abs(plain[..., -30:]).max(-1) > .3).all()
    check_rows(y, ref32, ref64, f"ends {flags}")
    for sl in (slice(0, 8), slice(-30, None)):              # the bar again on the edges alone: an error there cannot hide
        for b in range(2):
            for c in range(CH):
                assert np.abs(y[b, c, sl] - ref64[b, c, sl]).max() <= F.row_bound(ref32[b, c], ref64[b, c])


@pytest.mark.parametrize("flags", ["none", "both"])
def test_rows_longer_than_one_pass(dev, flags):
    """13500 samples at 160/147 are 12404 outputs = 85 frames: two full passes of 41 frames and a partial one, over four
    chunks of the chain kernel; the seams between passes carry no state, so any slip there shows as an error of order 1."""
    from rave_amd import data as D
    n, rng = 13500, np.random.default_rng(9)
    pcm = rng.integers(-30000, 30000, (2, CH, 14000)).astype(np.int16)
    nz = rng.random((2 * CH, n)).astype(np.float32)
    items, in_points, angles = [1, 0], [500, 0], [0.1, None]
    feed = D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=MAIN[0], seed=1, resample_to=MAIN[1], **FLAGS[flags])
    y = feed.sample(2, n, draws=(items, in_points, angles), noise=torch.from_numpy(nz)).cpu().numpy()
    assert y.shape == (2, CH, 12404) and 12404 == 84 * 147 + 56
    ref32, ref64 = (R.chain(pcm, nz, items, in_points, angles, *MAIN, variant=v, n=n, **FLAGS[flags]) for v in ("ref32", "ref64"))
    check_rows(y, ref32, ref64, f"three passes {flags}")


def test_pitched_and_muted_items_with_both_steps(pcm_d):
    feed = feed_of(pcm_d, MAIN, "both", rand_pitch=F.PITCH_RANGE)
    kw = dict(in_points=tuple(F.PITCH_IN_POINTS), ratios=tuple(F.RATIOS))
    y = run(feed, in_points=F.PITCH_IN_POINTS, ratios=F.RATIOS).cpu().numpy()
    check_rows(y, *reference(MAIN, "both", **kw), "pitched")
    mute = np.zeros(B, dtype=bool)
    mute[[0, 5]] = True                                     # a pitched, filtered item and a plain one
    for flags in ("both", "none"):                          # zeros stored by feed_post_kernel, and by the resampling kernel
        f = feed_of(pcm_d, MAIN, flags, rand_pitch=F.PITCH_RANGE)
        full = run(f, in_points=F.PITCH_IN_POINTS, ratios=F.RATIOS).cpu().numpy()
        z = run(f, in_points=F.PITCH_IN_POINTS, ratios=F.RATIOS, mute=mute).cpu().numpy()
        assert not z[mute].any() and full[mute].any()
        assert np.array_equal(z[~mute].view(np.uint32), full[~mute].view(np.uint32))


def _table(feed_mod, pcm_shape, angles=F.ANGLES, in_points=F.IN_POINTS):
    n_items, n_ch, length = pcm_shape
    t = np.zeros(B * n_ch, dtype=feed_mod.ROW_DTYPE)
    t["coef"] = np.nan
    t["length"] = length
    t["up"] = t["down"] = 1
    for b in range(B):
        for c in range(n_ch):
            row = t[b * n_ch + c]
            row["base"] = (int(F.ITEMS[b]) * n_ch + c) * length
            row["in_point"] = int(in_points[b])
            if angles[b] is not None:
                bb, aa = feed_mod.pole_to_z_filter(angles[b], .99)
                row["coef"] = [bb[0], bb[1], bb[2], aa[1], aa[2]]
    return t


class Entry:
    """The entry point itself on the test's batch, at 48000 -> 44100."""

    def __init__(self, dev, pcm_d, table):
        from rave_amd import _lib as L, data as D
        self.L, self.pcm_d, self.t = L, pcm_d, table
        self.t_d = torch.from_numpy(table.view(np.uint8)).to(dev)
        self.nz = torch.from_numpy(noise()).to(dev)
        taps, self.width = D.sinc_resample_kernel(*MAIN)
        self.taps = taps.contiguous().to(dev)
        self.n_res = R.resampled_length(N, *MAIN)
        self.need = L.lib.rh_feed_resample_workspace_bytes(B * CH, N, *MAIN)
        self.ws = torch.full((self.need // 8 + 1,), -3., device=dev, dtype=torch.float64)

    def __call__(self, out_ptr, rows=B * CH, n_ch=CH, norm=1, der=1, orig=MAIN[0], new=MAIN[1], n_taps=None, width=None, w=None,
                 w_bytes=None):
        L = self.L
        return L.lib.rh_feed_batch_resample_i16_f32(
            L.ptr(self.pcm_d), self.pcm_d.numel(), self.t.ctypes.data, L.ptr(self.t_d), None, 0, L.ptr(self.nz), rows, N, 16, n_ch,
            norm, 30.0, der, orig, new, L.ptr(self.taps), self.taps.numel() if n_taps is None else n_taps,
            self.width if width is None else width, L.ptr(self.ws) if w is None else w, self.need if w_bytes is None else w_bytes,
            out_ptr, L.stream())


def test_a_muted_channel_adds_nothing_to_the_items_peak(dev, pcm_d):
    """Channel 1 of the item that is loud in channel 1 only is muted in the row table (the feed mutes whole items): the row is
    zeros, and channel 0 is normalised by its own peak -- the row behind the muted one was never written and must not be read."""
    from rave_amd import _lib as L, data as D
    t = _table(D, pcm_d.shape)
    t["mute"][F.LOUD1 * CH + 1] = 1
    entry = Entry(dev, pcm_d, t)
    out = torch.full((B, CH, entry.n_res), 7., device=dev)
    entry.ws.fill_(float("nan"))                            # whatever a muted row's region holds
    L.check(entry(L.ptr(out)), "feed_batch_resample")
    y = out.cpu().numpy()
    assert np.isfinite(y).all() and not y[F.LOUD1, 1].any()
    item32, item64 = (R.resample(F.dequantized(F.make_pcm(), noise(), F.ITEMS, F.IN_POINTS, F.ANGLES, variant=v)[F.LOUD1], *MAIN, v)
                      for v in ("ref32", "ref64"))
    ref32, ref64 = (F.derivator(F.normalize_signal(x[0])) for x in (item32, item64))
    assert F.gain_of(np.abs(item64[0]).max()) > 4 * F.gain_of(np.abs(item64).max())
    err = float(np.abs(y[F.LOUD1, 0] - ref64).max())
    assert err <= F.row_bound(ref32.astype(np.float32), ref64), err
    others = np.delete(np.arange(B), F.LOUD1)
    assert np.array_equal(y[others], run(feed_of(pcm_d, MAIN, "both")).cpu().numpy()[others])


@pytest.mark.parametrize("flags", list(FLAGS))
def test_equal_rates_are_todays_feed(dev, pcm_d, flags):
    from rave_amd import _lib as L, data as D
    today = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, **FLAGS[flags])
    want = run(today)
    mute = [False, True, False, False, False, False]
    for to in (None, 44100):
        feed = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, resample_to=to, **FLAGS[flags])
        assert feed.resample_to is None and feed.res_taps is None
        assert torch.equal(run(feed), want) and torch.equal(run(feed, mute=mute), run(today, mute=mute))
        assert (feed.workspace is None) == (flags == "none")
        own = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, **FLAGS[flags])                      # own draws, same seed
        assert torch.equal(feed.sample(4, N), own.sample(4, N))
    # the entry point at equal rates: the bits of rh_feed_batch_post_i16_f32, its workspace, the table arguments not looked at
    entry = Entry(dev, pcm_d, _table(D, pcm_d.shape))
    out = torch.full((B, CH, N), 9., device=dev)
    kw = dict(norm=int("normalize" in FLAGS[flags]), der=int("derivative" in FLAGS[flags]))
    L.check(entry(L.ptr(out), orig=44100, new=44100, n_taps=0, width=0, w_bytes=L.lib.rh_feed_post_workspace_bytes(B * CH, N), **kw),
            "feed_batch_resample")
    assert torch.equal(out, want)


def test_same_call_twice_gives_the_same_bits(pcm_d):
    for rates, flags in ((MAIN, "none"), (MAIN, "both"), ((44100, 32000), "both")):
        feed = feed_of(pcm_d, rates, flags)
        y = run(feed)
        ws = feed.workspace
        assert torch.equal(run(feed), y) and feed.workspace is ws          # cached, not regrown
        small = run(feed, 1000, items=F.ITEMS[:2], in_points=F.IN_POINTS[:2], angles=F.ANGLES[:2])
        assert feed.workspace is ws and small.shape[-1] == R.resampled_length(1000, *rates)
        assert torch.equal(run(feed), y)


def test_frequency_masking_runs_on_the_resampled_rows(dev):
    """88200 -> 44100 at n_signal = 8192: the mask's length rule is met by the 4096 resampled samples, and the batch is the mask
    entry point applied to the unmasked resampled batch, bit for bit."""
    from rave_amd import _lib as L, data as D, ops
    pcm = torch.from_numpy(np.random.default_rng(5).integers(-20000, 20000, (4, CH, 9000)).astype(np.int16)).to(dev)
    items, in_points, angles = np.arange(4), np.array([0, 808, 5, 300]), [0.05, None, 0.2, None]
    bands = [None, (0, 1), (1969, 79), (300, 17)]
    nz = torch.from_numpy(np.random.default_rng(6).random((4 * CH, 8192)).astype(np.float32)).to(dev)
    for flags in ("none", "both"):
        kw = dict(sr=88200, seed=1, resample_to=44100, **FLAGS[flags])
        plain = D.GpuBatchFeed(pcm, **kw).sample(4, 8192, draws=(items, in_points, angles), noise=nz)
        got = D.GpuBatchFeed(pcm, freq_mask=.5, **kw).sample(4, 8192, draws=(items, in_points, angles), noise=nz, bands=bands)
        assert plain.shape == got.shape == (4, CH, 4096)
        table = torch.tensor([[0, 0] if b is None else list(b) for b in bands for _ in range(CH)], dtype=torch.int32, device=dev)
        want = torch.full_like(plain, 7.)
        L.check(L.lib.rh_feed_freq_mask_f32(L.ptr(plain), L.ptr(want), L.ptr(table), 4 * CH, 4096, L.ptr(ops._twiddle(4096, dev)),
                                            L.stream()), "feed_freq_mask")
        assert torch.equal(got, want) and torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])


@pytest.mark.parametrize("flags", ["none", "both"])
def test_out_that_is_only_4_byte_aligned(dev, pcm_d, flags):
    from rave_amd import _lib as L, data as D
    entry = Entry(dev, pcm_d, _table(D, pcm_d.shape))
    numel = B * CH * entry.n_res
    big = torch.full((numel + 4,), 7., device=dev)
    out = big[1:1 + numel]
    assert out.data_ptr() % 8 == 4
    kw = dict(norm=int(flags == "both"), der=int(flags == "both"))
    L.check(entry(out.data_ptr(), **kw), "feed_batch_resample")
    assert torch.equal(out.view(B, CH, -1), run(feed_of(pcm_d, MAIN, flags)))
    assert float(big[0]) == 7. and bool((big[1 + numel:] == 7.).all())


def test_refusals_launch_nothing(dev, pcm_d):
    from rave_amd import _lib as L, data as D
    entry = Entry(dev, pcm_d, _table(D, pcm_d.shape))
    out = torch.full((B, CH, entry.n_res), 7., device=dev)
    for kw in (dict(n_taps=entry.taps.numel() - 1), dict(n_taps=174), dict(width=entry.width + 1), dict(width=0),
               dict(w_bytes=entry.need - 8), dict(w=L.ptr(entry.ws) + 4), dict(rows=B * CH - 1), dict(n_ch=5), dict(orig=0)):
        with pytest.raises(RuntimeError):
            L.check(entry(L.ptr(out), **kw), "feed_batch_resample")
    torch.cuda.synchronize()
    assert bool((out == 7.).all()) and bool((entry.ws == -3.).all())
    L.check(entry(L.ptr(out)), "feed_batch_resample")      # the same arguments unharmed: runs, and leaves the spare word alone
    torch.cuda.synchronize()
    assert torch.equal(out, run(feed_of(pcm_d, MAIN, "both"))) and float(entry.ws[-1]) == -3.
