"""FrequencyMasking on the GPU (rh_feed_freq_mask_f32, ``GpuBatchFeed(freq_mask=...)``, rave_amd/data.py) against the
reference's expression in float64: scipy.signal.istft of the masked scipy.signal.stft (tests/feed_mask_model.py), behind the
reference chain restated with numpy / scipy (tests/feed_chain.py) for the whole feed.  The one bar is the project's parity
bar, relative L2 <= 1e-4 per row; a band misplaced by one bin moves a one-bin mask's result by about 3e-2."""
import numpy as np
import pytest
import torch

import feed_chain as F
import feed_mask_model as M

pytestmark = pytest.mark.gpu

ROWS = len(M.BANDS)
B, CH, LENGTH, N = 4, F.CH, 20000, 8192
ITEMS = np.array([2, 0, 3, 1])
ANGLES = [0.05, None, 0.2, None]
IN_POINTS = np.array([0, LENGTH - N, 777, 5])                      # both ends of the item
RATIOS = [(13, 10), None, (14, 19), None]
PITCH_IN_POINTS = np.array([26000 - N, LENGTH - N, 14737 - N, 5])   # ceil(20000 up / down) - N: the zero-padded far edge
FEED_BANDS = [None, (0, 1), (1969, 79), (300, 17)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def mask_rows(dev, x: np.ndarray, table) -> torch.Tensor:
    """The entry point on float32 rows; the result has one row more than x, which must come back untouched."""
    from rave_amd import _lib as L, ops
    n_rows, n = x.shape
    x_d = torch.from_numpy(x.astype(np.float32)).to(dev)
    y_d = torch.full((n_rows + 1, n), 7., device=dev)
    t_d = torch.tensor(table, dtype=torch.int32, device=dev).reshape(n_rows, 2)
    L.check(L.lib.rh_feed_freq_mask_f32(L.ptr(x_d), L.ptr(y_d), L.ptr(t_d), n_rows, n, L.ptr(ops._twiddle(M.NPERSEG, dev)), L.stream()),
            "feed_freq_mask")
    torch.cuda.synchronize()
    assert bool((y_d[n_rows] == 7.).all())
    return y_d[:n_rows]


@pytest.mark.parametrize("n", M.LENGTHS)
def test_entry_point_matches_scipy(dev, n):
    x = M.make_rows(ROWS, n)
    y = mask_rows(dev, x, M.BANDS)
    got = y.cpu().numpy()
    assert got.dtype == np.float32 and np.isfinite(got).all()
    for r, band in enumerate(M.BANDS):
        want = M.reference(x[r], band)
        err = M.rel_l2(got[r], want)
        print(f"n {n} row {r} band {band}: relative L2 {err:.3e} (removed {M.rel_l2(x[r], want):.3e} of the row)")
        assert err <= M.BAR, (n, r, band, err)
    # a row with no bins is its input, bit for bit; the other rows do not notice
    table = [list(b) for b in M.BANDS]
    table[2] = [123, 0]
    z = mask_rows(dev, x, table)
    assert torch.equal(z[2].cpu(), torch.from_numpy(x[2].astype(np.float32)))
    keep = [0, 1, 3, 4]
    assert torch.equal(z[keep], y[keep])
    assert torch.equal(mask_rows(dev, x, M.BANDS), y)               # the same bits on every run


def test_the_bar_tells_a_misplaced_band_and_holds_for_the_widest(dev):
    x = M.make_rows(2, 4096, seed=9)
    # an interior bin of white noise holds about 2 / 4096 of the energy: two different bins differ by about sqrt(4 / 4096) = 3e-2
    off = M.rel_l2(M.reference(x[0], (1001, 1)), M.reference(x[0], (1000, 1)))
    print(f"one-bin mask moved by one bin: relative L2 {off:.3e}")
    assert off > 10 * M.BAR
    # every bin below Nyquist (freq_mask_max_size = 2049): next to nothing is left of the row, so the transforms' float32
    # rounding, a fraction of the energy REMOVED, is held against the norm of the input rather than of the result
    got = mask_rows(dev, x, [(0, 2048), (1, 2047)]).cpu().numpy().astype(np.float64)
    for r, band in enumerate([(0, 2048), (1, 2047)]):
        want = M.reference(x[r], band)
        err = float(np.linalg.norm(got[r] - want) / np.linalg.norm(x[r]))
        print(f"band {band}: |got - scipy| / |x| {err:.3e}, |scipy| / |x| {np.linalg.norm(want) / np.linalg.norm(x[r]):.3e}")
        assert err <= M.BAR, (band, err)


@pytest.fixture(scope="module")
def pcm():
    rng = np.random.default_rng(4)
    x = rng.integers(-12000, 12000, size=(B, CH, LENGTH)) + np.array([3000, -5000])[None, :, None]
    return x.astype(np.int16)


@pytest.fixture(scope="module")
def pcm_d(dev, pcm):
    return torch.from_numpy(pcm).to(dev)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(2).random((B * CH, N)).astype(np.float32)


CASES = {"plain": (dict(), dict(in_points=IN_POINTS, ratios=None, mute=None)),
         "combined": (dict(rand_pitch=F.PITCH_RANGE, normalize=True, derivative=True),
                      dict(in_points=PITCH_IN_POINTS, ratios=RATIOS, mute=[False, False, False, True]))}


@pytest.mark.parametrize("case", list(CASES))
def test_whole_feed_matches_the_reference_chain(dev, pcm, pcm_d, noise, case):
    from rave_amd import data as D
    kw, d = CASES[case]
    draws = (ITEMS, d["in_points"], ANGLES) if d["ratios"] is None else (ITEMS, d["in_points"], ANGLES, d["ratios"])
    nz = torch.from_numpy(noise).to(dev)
    feed = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, freq_mask=.5, **kw)
    y = feed.sample(B, N, draws=draws, noise=nz, mute=d["mute"], bands=FEED_BANDS)
    assert y.shape == (B, CH, N) and y.dtype == torch.float32 and feed.mask_input is not None
    without = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, **kw).sample(B, N, draws=draws, noise=nz, mute=d["mute"])
    assert torch.equal(y[0], without[0])                            # the item that is not masked: the bits of the feed without
    assert not torch.equal(y[1], without[1])
    ref = F.chain(pcm, noise, ITEMS, d["in_points"], ANGLES, d["ratios"], d["mute"], normalize=kw.get("normalize", False),
                  derivative=kw.get("derivative", False), variant="ref64", n=N)
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    for b in range(B):
        if d["mute"] is not None and d["mute"][b]:
            assert not got[b].any() and FEED_BANDS[b] is not None   # a muted item stays silent under its mask
            continue
        want = M.reference(ref[b], FEED_BANDS[b]).astype(np.float32)       # both channels of the item, the item's band
        for c in range(CH):
            err = M.rel_l2(got[b, c], want[c].astype(np.float64))
            print(f"{case} item {b}.{c} band {FEED_BANDS[b]}: relative L2 {err:.3e}")
            assert err <= M.BAR, (case, b, c, err)
    # the same call again: the same bits, the cached buffer kept
    buf = feed.mask_input
    assert torch.equal(feed.sample(B, N, draws=draws, noise=nz, mute=d["mute"], bands=FEED_BANDS), y) and feed.mask_input is buf


def test_no_item_masked_is_the_feed_without_the_option(dev, pcm_d, noise):
    from rave_amd import data as D
    nz = torch.from_numpy(noise).to(dev)
    draws = (ITEMS, IN_POINTS, ANGLES)
    plain = D.GpuBatchFeed(pcm_d, sr=44100, seed=1)
    want = plain.sample(B, N, draws=draws, noise=nz)
    feed = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, freq_mask=.5)
    assert torch.equal(feed.sample(B, N, draws=draws, noise=nz, bands=[None] * B), want)
    assert torch.equal(feed.sample(B, N, draws=draws, noise=nz), want)              # injected draws: no band is drawn
    assert feed.mask_input is None                                  # no buffer: the chain wrote the batch, nothing followed
    never = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, freq_mask=0.)                   # own draws, same seed: never a mask
    assert torch.equal(never.sample(B, N), D.GpuBatchFeed(pcm_d, sr=44100, seed=1).sample(B, N)) and never.mask_input is None
    always = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, freq_mask=1., freq_mask_max_size=2)
    a, b = always.sample(B, N), D.GpuBatchFeed(pcm_d, sr=44100, seed=1).sample(B, N)
    assert always.mask_input is not None and not torch.equal(a, b)  # the same chain draws, every item less one bin
