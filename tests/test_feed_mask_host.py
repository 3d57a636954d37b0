"""Host side of the data feed's ``freq_mask`` option (rave_amd/data.py, rh_feed_freq_mask_f32): the identity the kernel rests on
(tests/feed_mask_model.py against scipy.signal.stft / istft), the draws, the arguments ``GpuBatchFeed`` refuses and the entry
point's refusals (host checks, nothing is launched)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import feed_mask_model as M


class HostPcm:
    """Stand-in for the resident PCM, so that a feed can be built without a GPU: the constructor and ``draw`` look at nothing
    but its type, its shape and its device."""
    dtype, is_cuda, device = torch.int16, True, torch.device("cpu")

    def __init__(self, n_items=64, n_ch=2, length=20000):
        self.shape = (n_items, n_ch, length)

    def dim(self):
        return 3

    def contiguous(self):
        return self


@pytest.mark.parametrize("n", M.LENGTHS)
def test_formulation_equals_istft_of_the_masked_stft(n):
    """x minus the band component, block by block from two frames, is scipy's istft(mask(stft(x))): 1e-12 absolute on
    unit-variance noise, for every band of the GPU test, and the output has exactly n samples."""
    x = M.make_rows(2, n)
    assert abs(float(x.std()) - 1) < .05
    for band in M.BANDS:
        want = M.reference(x, band)
        assert want.shape == x.shape and want.dtype == np.float64
        err = float(np.abs(M.model(x, band) - want).max())
        print(f"n {n} band {band}: max |model - scipy| {err:.3e}, removed {M.rel_l2(x, want):.3e} of the row")
        assert err <= 1e-12, (n, band, err)
        assert M.rel_l2(x, want) > 1e-3                     # the mask did something
    assert M.model(x, None) is x and M.reference(x, None) is x


def test_draws_follow_the_reference_distributions():
    from rave_amd import data as D
    bands = D.draw_bands(np.random.default_rng(11), 4000, .5, 80)
    assert len(bands) == 4000
    masked = [b for b in bands if b is not None]
    for freq_idx, mask_size in masked:
        assert 1 <= mask_size <= 79 and 0 <= freq_idx <= 2048 - mask_size
    sizes = {b[1] for b in masked}
    assert 1 in sizes and 79 in sizes
    share = len(masked) / 4000
    print(f"masked share {share:.4f}, freq_idx in [{min(b[0] for b in masked)}, {max(b[0] for b in masked)}]")
    assert abs(share - .5) <= .04                           # 5 sigma of a Bernoulli(.5) mean over 4000
    assert D.draw_bands(np.random.default_rng(11), 50, 0., 80) == [None] * 50
    assert all(b is not None for b in D.draw_bands(np.random.default_rng(11), 50, 1., 80))
    assert {b[1] for b in D.draw_bands(np.random.default_rng(11), 50, 1., 2)} == {1}


def test_a_feed_without_the_option_draws_as_before():
    from rave_amd import data as D
    sig = inspect.signature(D.GpuBatchFeed.__init__).parameters
    assert sig["freq_mask"].default is None and sig["freq_mask_max_size"].default == 80
    assert "bands" in inspect.signature(D.GpuBatchFeed.sample).parameters
    pcm = HostPcm()
    feeds = [D.GpuBatchFeed(pcm, seed=5), D.GpuBatchFeed(pcm, seed=5, freq_mask=None), D.GpuBatchFeed(pcm, seed=5, freq_mask=0.),
             D.GpuBatchFeed(pcm, seed=5, freq_mask=.5)]
    for _ in range(3):                                      # draw() itself never touches the bands: the sequences stay in step
        draws = [f.draw(16, 8192) for f in feeds]
        for d in draws[1:]:
            assert len(d) == len(draws[0]) == 3
            assert np.array_equal(d[0], draws[0][0]) and np.array_equal(d[1], draws[0][1]) and d[2] == draws[0][2]
    # and the generator of a feed without the option is where draw_batch alone leaves it
    rng = np.random.default_rng(5)
    for _ in range(3):
        D.draw_batch(rng, 64, 20000, 16, 8192, 44100, .8, None)
    assert feeds[0].rng.random() == feeds[1].rng.random() == rng.random()


def test_bad_arguments_raise():
    from rave_amd import data as D
    pcm = HostPcm()
    host = torch.zeros(1, 1, 8, dtype=torch.int16)          # refused before the PCM is looked at
    for bad in (-.1, 1.1, float("nan")):
        for p in (pcm, host):
            with pytest.raises(RuntimeError, match="freq_mask"):
                D.GpuBatchFeed(p, freq_mask=bad)
    for bad in (1, 0, -3, 2050):
        for p in (pcm, host):
            with pytest.raises(RuntimeError, match="freq_mask_max_size"):
                D.GpuBatchFeed(p, freq_mask=.5, freq_mask_max_size=bad)
    for ok in (2, 80, 2049):
        D.GpuBatchFeed(pcm, freq_mask=.5, freq_mask_max_size=ok)
    D.GpuBatchFeed(pcm, freq_mask=0.), D.GpuBatchFeed(pcm, freq_mask=1.)
    feed = D.GpuBatchFeed(pcm, freq_mask=.5)
    for n in (2048, 4095, 4097, 10000, 6000):               # lengths scipy would pad, or shorten the window for
        with pytest.raises(RuntimeError, match="multiple of 2048"):
            feed.sample(4, n)
        with pytest.raises(RuntimeError, match="multiple of 2048"):
            feed.sample(4, n, bands=[None] * 4)
    draws = (np.arange(4), np.zeros(4, dtype=np.int64), [None] * 4)
    for bad in ((0, 0), (5, -1), (-1, 3), (2048, 1), (2000, 49), (0, 2049)):
        with pytest.raises(RuntimeError, match="band"):
            feed.sample(4, 8192, draws=draws, bands=[None, bad, None, None])
    with pytest.raises(RuntimeError, match="bands for a batch"):
        feed.sample(4, 8192, draws=draws, bands=[(0, 1)] * 3)
    with pytest.raises(RuntimeError, match="without freq_mask"):
        D.GpuBatchFeed(pcm).sample(4, 8192, draws=draws, bands=[(0, 1)] * 4)
    assert D.check_bands([None, (0, 2048), (2047, 1)], 3) is not None and D.check_bands([None] * 3, 3) is None


def test_entry_point_refuses_on_the_host_without_a_launch():
    """No GPU here: a call that got as far as a launch would fail with another message than the ones matched below."""
    from rave_amd import _lib as L
    n_rows, n = 2, 4096
    buf = (C.c_float * (2 * n_rows * n + 4))()
    x = C.addressof(buf)
    y = x + 4 * n_rows * n
    tw = (C.c_double * 4096)()                              # 8-byte aligned storage for the table
    table = (C.c_int32 * (2 * n_rows))()
    t, bands = C.addressof(tw), C.addressof(table)

    def call(x=x, y=y, bands=bands, rows=n_rows, n=n, t=t):
        return L.lib.rh_feed_freq_mask_f32(x, y, bands, rows, n, t, None)

    for kw, word in ((dict(x=None), b"null"), (dict(y=None), b"null"), (dict(bands=None), b"null"), (dict(t=None), b"null"),
                     (dict(rows=0), b"rows"), (dict(rows=-1), b"rows"), (dict(n=2048), b"n_signal"), (dict(n=0), b"n_signal"),
                     (dict(n=4095), b"n_signal"), (dict(n=4097), b"n_signal"), (dict(n=10000), b"n_signal"), (dict(n=-4096), b"n_signal"),
                     (dict(t=t + 4), b"8-byte"), (dict(y=x), b"overlap"), (dict(y=x + 4), b"overlap"),
                     (dict(y=y - 4), b"overlap"), (dict(x=y, y=x + 4), b"overlap")):
        assert call(**kw) == -1 and word in L.lib.rh_last_error(), (kw, L.lib.rh_last_error())      # RH_ERR_INVALID
