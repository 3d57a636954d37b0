"""``GpuBatchFeed(normalize=..., derivative=...)`` (rh_feed_batch_post_i16_f32, rave_amd/data.py) against the reference's chain
restated with numpy / scipy (tests/feed_chain.py) on injected draws: 6 stereo items x 6000 samples, batch 6, n_signal = 4352 =
one full 4096-sample chunk of the chain kernel plus a ragged one (two full 2048-sample tiles of the second kernel plus a ragged
one), so both the item's peak and the derivator's x[n - 1] cross a seam.  The one bar, per row (tests/test_gpu_feed_pitch.py):
    max |got - ref64| <= 2 max |ref32 - ref64| + 2^-23 max |ref64|."""
import numpy as np
import pytest
import torch

import feed_chain as F

pytestmark = pytest.mark.gpu

B, CH, N = F.N_ITEMS, F.CH, F.N
FLAGS = {"normalize": dict(normalize=True), "derivative": dict(derivative=True), "both": dict(normalize=True, derivative=True)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pcm():
    return F.make_pcm()


@pytest.fixture(scope="module")
def pcm_d(dev, pcm):
    return torch.from_numpy(pcm).to(dev)


@pytest.fixture(scope="module")
def noise():
    return F.make_noise()


@pytest.fixture(scope="module")
def feeds(pcm_d):
    from rave_amd import data as D
    out = {k: D.GpuBatchFeed(pcm_d, sr=44100, seed=1, **kw) for k, kw in FLAGS.items()}
    out["plain"] = D.GpuBatchFeed(pcm_d, sr=44100, seed=1)
    return out


def run(feed, noise, angles=F.ANGLES, in_points=F.IN_POINTS, ratios=None, mute=None):
    draws = (F.ITEMS, in_points, angles) if ratios is None else (F.ITEMS, in_points, angles, ratios)
    y = feed.sample(B, N, draws=draws, noise=torch.from_numpy(noise), mute=mute).cpu().numpy()
    assert y.shape == (B, CH, N) and y.dtype == np.float32
    return y


@pytest.fixture(scope="module")
def plain(feeds, noise):
    return run(feeds["plain"], noise)


@pytest.fixture(scope="module")
def got(feeds, noise):
    return {k: run(feeds[k], noise) for k in FLAGS}


def check_rows(got, ref32, ref64, what):
    for b in range(got.shape[0]):
        for c in range(CH):
            err = float(np.abs(got[b, c].astype(np.float64) - ref64[b, c]).max())
            bound = F.row_bound(ref32[b, c], ref64[b, c])
            print(f"{what} row {b}.{c}: err {err:.3e} bound {bound:.3e} (max |ref| {np.abs(ref64[b, c]).max():.3e})")
            assert np.isfinite(got[b, c]).all() and err <= bound, (what, b, c, err, bound)


@pytest.mark.parametrize("angles", [F.ANGLES, F.ANGLES_FLIPPED], ids=["allpass-024", "allpass-135"])
@pytest.mark.parametrize("flags", list(FLAGS))
def test_steps_match_the_reference_chain(feeds, pcm, noise, flags, angles):
    y = run(feeds[flags], noise, angles)
    ref = {v: F.chain(pcm, noise, F.ITEMS, F.IN_POINTS, angles, variant=v, **FLAGS[flags]) for v in ("ref32", "ref64")}
    check_rows(y, ref["ref32"], ref["ref64"], flags)


def test_gain_is_item_wide(pcm, noise, got, plain):
    """Channel 0 of the item that is loud in channel 1 only: got = float32(v g) and plain = float32(v) with g from the peak of
    channel 1, so |got - plain g| <= 2 * 2^-24 |v g| (two float32 roundings); a per-row peak gives channel 0 the capped gain."""
    item = F.dequantized(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES)[F.LOUD1]
    row_peaks = np.abs(item).max(-1)
    assert row_peaks[1] > 10 * row_peaks[0]
    g = float(F.gain_of(row_peaks[1]))
    want = plain[F.LOUD1, 0].astype(np.float64) * g
    err = np.abs(got["normalize"][F.LOUD1, 0].astype(np.float64) - want)
    assert (err <= 1.0001 * 2.0 ** -23 * np.abs(want)).all(), float((err / np.abs(want)).max())
    ratio = got["normalize"][F.LOUD1, 0].astype(np.float64) / plain[F.LOUD1, 0]
    print(f"gain {g:.6f}, got / plain in [{ratio.min():.6f}, {ratio.max():.6f}], per-row gain would be {F.gain_of(row_peaks[0]):.3f}")


def test_cap_and_zero(feeds, pcm, noise, got, plain):
    ref = {v: F.chain(pcm, noise, F.ITEMS, F.IN_POINTS, F.ANGLES, variant=v, normalize=True) for v in ("ref32", "ref64")}
    capped = plain[F.QUIET].astype(np.float64) * 10 ** 1.5
    for c in range(CH):
        err = float(np.abs(got["normalize"][F.QUIET, c] - capped[c]).max())
        assert err <= F.row_bound(ref["ref32"][F.QUIET, c], ref["ref64"][F.QUIET, c]), (c, err)
    zero = np.zeros_like(noise)
    for k in FLAGS:                                     # log10(0) is never taken: no NaN, no -0 * inf
        for angles in (F.ANGLES, F.ANGLES_FLIPPED):     # the all-zero item with the all-pass off and on
            y = run(feeds[k], zero, angles)
            assert np.isfinite(y).all() and not y[F.ZERO].any(), k
            assert y[F.FULL].any()


def test_derivative_crosses_the_chunk_seam(got, plain):
    """Derivative alone: got[n] = float32(0.5 v[n] - 0.5 v[n - 1]) on the unrounded v, plain = float32(v); the two roundings of
    plain and the one of got add up to at most 2^-23 max(|v[n]|, |v[n - 1]|): one float32 ulp at the size of the operands.
    n = 4096 is the first sample of the chain kernel's second chunk (and of the second kernel's third tile), 2048 a tile seam
    of the second kernel alone; sample 0 has no predecessor and 0.5 x is exact."""
    y, x = got["derivative"].astype(np.float64), plain.astype(np.float64)
    assert np.array_equal(got["derivative"][..., 0], 0.5 * plain[..., 0])
    for n in (4096, 2048, 4095, 4097, N - 1):
        want = 0.5 * (x[..., n] - x[..., n - 1])
        tol = 2.0 ** -23 * np.maximum(np.abs(x[..., n]), np.abs(x[..., n - 1]))
        assert (np.abs(y[..., n] - want) <= tol).all(), n
    busy = np.delete(np.arange(B), F.ZERO)
    assert (np.abs(x[busy][..., 4095]) > 2.0 ** -16).all()     # a dropped predecessor would be far outside


def test_pitched_and_muted_items_with_both_steps(pcm_d, pcm, noise):
    from rave_amd import data as D
    kw = dict(normalize=True, derivative=True)
    feed = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, rand_pitch=F.PITCH_RANGE, **kw)
    args = (F.ITEMS, F.PITCH_IN_POINTS, F.ANGLES, F.RATIOS)
    y = run(feed, noise, F.ANGLES, F.PITCH_IN_POINTS, F.RATIOS)
    ref = {v: F.chain(pcm, noise, *args, variant=v, **kw) for v in ("ref32", "ref64")}
    check_rows(y, ref["ref32"], ref["ref64"], "pitched")
    mute = np.zeros(B, dtype=bool)
    mute[[0, 5]] = True                                 # a pitched, filtered item and a plain one
    z = run(feed, noise, F.ANGLES, F.PITCH_IN_POINTS, F.RATIOS, mute=mute)
    assert not z[mute].any() and y[mute].any()
    assert np.array_equal(z[~mute].view(np.uint32), y[~mute].view(np.uint32))


def _table(feed_mod, pcm_shape, angles, in_points):
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


def test_flags_off_is_todays_feed(dev, pcm_d, noise, feeds, plain):
    from rave_amd import _lib as L, data as D
    nz = torch.from_numpy(noise).to(dev)
    off = D.GpuBatchFeed(pcm_d, sr=44100, seed=1, normalize=False, derivative=False)
    draws = (F.ITEMS, F.IN_POINTS, F.ANGLES)
    assert torch.equal(off.sample(B, N, draws=draws, noise=nz), feeds["plain"].sample(B, N, draws=draws, noise=nz))
    assert off.workspace is None
    mute = [False, True, False, False, False, False]    # the table path (rh_feed_batch_pitch_i16_f32)
    assert torch.equal(off.sample(B, N, draws=draws, noise=nz, mute=mute), feeds["plain"].sample(B, N, draws=draws, noise=nz, mute=mute))
    assert torch.equal(off.sample(4, N), D.GpuBatchFeed(pcm_d, sr=44100, seed=1).sample(4, N))       # own draws, same seed
    # the entry point itself with both steps off: the bits of rh_feed_batch_pitch_i16_f32, no workspace
    t = _table(D, pcm_d.shape, F.ANGLES, F.IN_POINTS)
    t["mute"][2:4] = 1
    t_d = torch.from_numpy(t.view(np.uint8)).to(dev)
    a, b = torch.full((B, CH, N), 7., device=dev), torch.full((B, CH, N), 9., device=dev)
    L.check(L.lib.rh_feed_batch_pitch_i16_f32(L.ptr(pcm_d), pcm_d.numel(), t.ctypes.data, L.ptr(t_d), None, 0, L.ptr(nz), B * CH, N,
                                              16, L.ptr(a), L.stream()), "feed_batch_pitch")
    L.check(L.lib.rh_feed_batch_post_i16_f32(L.ptr(pcm_d), pcm_d.numel(), t.ctypes.data, L.ptr(t_d), None, 0, L.ptr(nz), B * CH, N,
                                             16, CH, 0, 30.0, 0, None, 0, L.ptr(b), L.stream()), "feed_batch_post")
    assert torch.equal(a, b) and not bool(a[1].any()) and torch.equal(a.cpu(), torch.from_numpy(plain) * (1 - torch.tensor(t["mute"][::CH]).view(B, 1, 1).float()))


def test_same_call_twice_gives_the_same_bits(dev, feeds, noise, got):
    nz = torch.from_numpy(noise).to(dev)
    for k in FLAGS:
        ws = feeds[k].workspace
        y = feeds[k].sample(B, N, draws=(F.ITEMS, F.IN_POINTS, F.ANGLES), noise=nz)
        assert feeds[k].workspace is ws                 # cached, not regrown
        assert torch.equal(y.cpu(), torch.from_numpy(got[k]))
        small = feeds[k].sample(2, 1000, draws=(F.ITEMS[:2], F.IN_POINTS[:2], F.ANGLES[:2]), noise=nz[:4, :1000].contiguous())
        assert feeds[k].workspace is ws and small.shape == (2, CH, 1000)
        assert torch.equal(feeds[k].sample(B, N, draws=(F.ITEMS, F.IN_POINTS, F.ANGLES), noise=nz), y)


def test_refusals_launch_nothing(dev, pcm_d, noise, feeds):
    from rave_amd import _lib as L, data as D
    nz = torch.from_numpy(noise).to(dev)
    t = _table(D, pcm_d.shape, F.ANGLES, F.IN_POINTS)
    t_d = torch.from_numpy(t.view(np.uint8)).to(dev)
    need = L.lib.rh_feed_post_workspace_bytes(B * CH, N)
    ws = torch.full((need // 8 + 1,), -3., device=dev, dtype=torch.float64)
    out = torch.full((B, CH, N), 7., device=dev)

    def call(rows=B * CH, n_ch=CH, cap=30.0, w=L.ptr(ws), w_bytes=need):
        return L.lib.rh_feed_batch_post_i16_f32(L.ptr(pcm_d), pcm_d.numel(), t.ctypes.data, L.ptr(t_d), None, 0, L.ptr(nz), rows, N, 16,
                                                n_ch, 1, cap, 1, w, w_bytes, L.ptr(out), L.stream())

    for kw in (dict(rows=B * CH - 1), dict(n_ch=5), dict(w_bytes=need - 8), dict(w=L.ptr(ws) + 4), dict(cap=float("nan")),
               dict(cap=float("inf"))):
        with pytest.raises(RuntimeError):
            L.check(call(**kw), "feed_batch_post")
    torch.cuda.synchronize()
    assert bool((out == 7.).all()) and bool((ws == -3.).all())
    with pytest.raises(RuntimeError):
        D.GpuBatchFeed(pcm_d, normalize=True, max_gain_db=float("nan"))
    L.check(call(), "feed_batch_post")                  # the same arguments unharmed: runs, and leaves the spare word alone
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(run(feeds["both"], noise))) and float(ws[-1]) == -3.
