"""The pitched data feed on the GPU (rh_feed_batch_pitch_i16_f32, rave_amd/data.py) against the reference's chain restated
with scipy: int16 -> float32, RandomPitch = scipy.signal.resample_poly(padtype='mean') of the whole item
(rave/transforms.py:56-89), RandomCrop, the all-pass phase mangle through lfilter (rave/dataset.py:283-299),
Dequantize(16), RandomMute (rave/transforms.py:168-177), float32 -- on injected draws."""
import numpy as np
import pytest
import torch
from scipy.signal import lfilter, resample_poly

pytestmark = pytest.mark.gpu

LENGTH, N = 9001, 4100          # n_signal crosses the 4096-sample chunk seam: staged span, tap phases, filter state
RANGE = (0.6, 1.4)              # holds 19/14 (the longest filter) and 4/6
ITEMS = np.array([3, 0, 4, 1, 2, 3, 0])
RATIOS = [(19, 14), (13, 10), (7, 10), (14, 19), (18, 19), None, (4, 6)]
ANGLES = [0.05, None, 0.2, None, 0.003, 0.1, 0.7]
BATCH = len(RATIOS)


def n_out(ratio):
    return LENGTH if ratio is None else -(-LENGTH * ratio[0] // ratio[1])          # resample_poly: ceil(L up / down)


# both zero-padded edges (0 and n_out - n_signal) and interior odd crop points
IN_POINTS = np.array([0, n_out(RATIOS[1]) - N, 1111, n_out(RATIOS[3]) - N, 777, LENGTH - N, n_out(RATIOS[6]) - N])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pcm():
    rng = np.random.default_rng(0)
    x = rng.integers(-12000, 12000, size=(5, 2, LENGTH)) + np.array([5000, -7000])[None, :, None]     # DC offset per channel
    return x.astype(np.int16)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(1).random((BATCH * 2, N)).astype(np.float32)


def chain(pcm, noise, angles, dtype):
    """The reference chain for the injected draws, RandomPitch evaluated in ``dtype`` (upstream: float32, since
    resample_poly casts its filter to the dtype of the item); (BATCH, 2, N) float64, before the last astype."""
    out = np.empty((BATCH, 2, N), dtype=np.float64)
    for b in range(BATCH):
        x = (pcm[ITEMS[b]].astype(np.float32) / (2 ** 15 - 1)).astype(dtype)
        if RATIOS[b] is not None:
            x = resample_poly(x, RATIOS[b][0], RATIOS[b][1], padtype="mean", axis=-1)
            assert x.dtype == dtype and x.shape[-1] == n_out(RATIOS[b])
        x = x[..., IN_POINTS[b]:IN_POINTS[b] + N]
        if angles[b] is not None:
            z0 = .99 * np.exp(1j * angles[b])                                      # rave/dataset.py:290-294
            aa = [1.0, -2.0 * float(np.real(z0)), float(abs(z0) ** 2)]
            bb = [float(abs(z0) ** 2), -2.0 * float(np.real(z0)), 1.0]
            x = lfilter(bb, aa, x)
        out[b] = x.astype(np.float64) + noise[2 * b:2 * b + 2].astype(np.float64) / 2 ** 16
    return out


@pytest.fixture(scope="module")
def feed(dev, pcm):
    from rave_amd import data as D
    return D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=44100, seed=1, rand_pitch=RANGE)


@pytest.fixture(scope="module")
def got(feed, noise):
    return feed.sample(BATCH, N, draws=(ITEMS, IN_POINTS, ANGLES, RATIOS), noise=torch.from_numpy(noise)).cpu().numpy()


def test_pitched_feed_matches_the_reference_chain(pcm, noise, got):
    """Per row max|got - ref64| <= max|ref32 - ref64| + 2e-6 max(1, max|ref|): the reference's own float32 deviation,
    measured here, plus the bound of the unpitched feed's parity test."""
    ref32 = chain(pcm, noise, ANGLES, np.float32).astype(np.float32)
    ref64 = chain(pcm, noise, ANGLES, np.float64)
    assert got.shape == (BATCH, 2, N) and got.dtype == np.float32
    for b in range(BATCH):
        for c in range(2):
            own = np.abs(ref32[b, c].astype(np.float64) - ref64[b, c]).max()
            err = np.abs(got[b, c].astype(np.float64) - ref64[b, c]).max()
            bound = own + 2e-6 * max(1.0, np.abs(ref64[b, c]).max())
            print(f"row {b}.{c} ratio {RATIOS[b]}: err {err:.3e} reference's own {own:.3e} bound {bound:.3e}")
            assert err <= bound, (b, c, RATIOS[b])


def test_resampler_alone_is_within_the_float32_rounding_of_the_reference(feed, pcm):
    """All-pass off, zero noise: max|got - ref64| <= 2 max|ref32 - ref64| + 2^-23 max|ref| per row -- wrong taps, a phase off
    by one or a wrong mean (the items carry a DC offset, the crops touch both zero-padded edges) are far outside."""
    off = [None] * BATCH
    zero = np.zeros((BATCH * 2, N), dtype=np.float32)
    got = feed.sample(BATCH, N, draws=(ITEMS, IN_POINTS, off, RATIOS), noise=torch.from_numpy(zero)).cpu().numpy()
    ref32 = chain(pcm, zero, off, np.float32)
    ref64 = chain(pcm, zero, off, np.float64)
    for b in range(BATCH):
        for c in range(2):
            own = np.abs(ref32[b, c] - ref64[b, c]).max()
            err = np.abs(got[b, c].astype(np.float64) - ref64[b, c]).max()
            bound = 2 * own + 2.0 ** -23 * np.abs(ref64[b, c]).max()
            print(f"row {b}.{c} ratio {RATIOS[b]}: err {err:.3e} reference's own {own:.3e} bound {bound:.3e}")
            assert err <= bound, (b, c, RATIOS[b])


def test_muted_item_is_exactly_zero_and_the_others_do_not_move(feed, noise, got):
    mute = np.zeros(BATCH, dtype=bool)
    mute[2] = True
    y = feed.sample(BATCH, N, draws=(ITEMS, IN_POINTS, ANGLES, RATIOS), noise=torch.from_numpy(noise), mute=mute).cpu().numpy()
    assert not y[2].any()
    keep = ~mute
    assert np.array_equal(y[keep], got[keep]) and got[2].any()
    # RandomMute without RandomPitch goes through the same entry point
    plain = feed.sample(2, N, draws=(ITEMS[4:6], np.array([5, LENGTH - N]), ANGLES[4:6]), noise=torch.from_numpy(noise[:4]),
                        mute=[True, False]).cpu().numpy()
    ref = feed.sample(2, N, draws=(ITEMS[4:6], np.array([5, LENGTH - N]), ANGLES[4:6]), noise=torch.from_numpy(noise[:4])).cpu().numpy()
    assert not plain[0].any() and np.array_equal(plain[1], ref[1])


def test_unpitched_row_is_bit_identical_to_the_plain_feed(dev, pcm, noise, got):
    from rave_amd import data as D
    b = RATIOS.index(None)
    plain = D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=44100, seed=1)
    ref = plain.sample(1, N, draws=(ITEMS[b:b + 1], IN_POINTS[b:b + 1], ANGLES[b:b + 1]),
                       noise=torch.from_numpy(noise[2 * b:2 * b + 2])).cpu().numpy()
    assert np.array_equal(ref[0].view(np.uint32), got[b].view(np.uint32))


def test_feed_draws_its_own_pitched_batches(dev, pcm):
    from rave_amd import data as D
    feed = D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=44100, seed=5, rand_pitch=(0.7, 1.3), p_mute=.25)
    draws = feed.draw(16, N)
    assert len(draws) == 4 and any(r is not None for r in draws[3]) and any(r is None for r in draws[3])
    y = feed.sample(16, N)
    assert y.shape == (16, 2, N) and bool(torch.isfinite(y).all()) and float(y.abs().max()) < 4.0
    silent = (y == 0).all(-1).all(-1)
    assert 0 < int(silent.sum()) < 16                                              # p_mute = .25 over 16 items, seed 5
    with pytest.raises(RuntimeError):                                              # 9001 * 0.7 < 6400
        feed.draw(4, 6400)


@pytest.mark.parametrize("ratio,in_point", [((20, 19), 0), ((19, 20), 0), ((0, 3), 0), ((3, 0), 0), ((-2, 3), 0),
                                            ((13, 10), n_out((13, 10)) - N + 1), ((7, 10), -1), ((7, 10), LENGTH - N)])
def test_bad_ratio_or_window_is_an_error(feed, noise, ratio, in_point):
    with pytest.raises(RuntimeError):
        feed.sample(1, N, draws=(ITEMS[:1], np.array([in_point]), [None], [ratio]), noise=torch.from_numpy(noise[:2]))
        torch.cuda.synchronize()
