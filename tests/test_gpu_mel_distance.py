"""GPU tests of the differentiable mel spectrogram (rave_amd/csrc/mel.hip: rh_mel_diff_fwd_f32 / rh_mel_diff_bwd_f32,
rave_amd.ops.mel_spectrogram_diff, rave_amd.mel.DifferentiableMelSpectrogram) and of the mel variant of ``SpectralDistance`` on
it: both directions against the float64 restatement of tests/mel_distance_reference.py (computed on the CPU, once per case) at
the project's parity bar -- relative L2 <= 1e-4, forward overall AND per mel channel as tests/test_gpu_mel.py holds the same
kernel to, backward as tests/test_gpu_spectrogram.py holds the adjoint it is modelled on -- the edges (a silent row, the
uncovered tail, repeatability), pointers that are only 4-byte aligned, a recorded step, and the loss end to end.  Measured on the
MI355X over the cases below: forward 7e-8 .. 5e-7 overall (worst mel channel 7.5e-7), backward 1.6e-7 .. 4.1e-7, power 1 no
worse than power 2, so the fallback bound the power-1 backward was allowed (twice the float32 composition's own error) is not
used; the loss end to end: values 1e-8 .. 1e-7, grad_y 4e-7 .. 9e-7 of float64 (profiles/mel_distance.txt)."""
from functools import partial

import pytest
import torch

import mel_distance_reference as R
from conftest import rel_l2
from test_gpu_mel import BAR, _per_channel

pytestmark = pytest.mark.gpu

SR = 44100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# (n_fft, hop, T, rows, n_mels, power, normalized, center): n_fft = the smallest, a middle and the largest size of the dispatch;
# hop = n_fft / 4 and one that does not divide T - n_fft; T = n_fft (one frame uncentred) and 3 n_fft + 5 (a tail no frame
# covers); rows 1 and 3; 1, 16 and 128 filters (128 over the 65 bins of n_fft = 128: most filters are empty); and one T per size
# that takes more than one workgroup in either direction (a backward span is 2048 samples up to n_fft = 512 and 8192 at 2048).
CASES = [
    (128, 32, 128, 1, 128, 1, True, False), (128, 32, 389, 3, 128, 2, False, False), (128, 32, 389, 3, 16, 1, True, True),
    (128, 50, 389, 1, 1, 2, True, False), (128, 32, 128, 3, 16, 2, True, True), (128, 32, 5000, 3, 16, 1, True, False),
    (512, 128, 512, 1, 16, 1, False, False), (512, 128, 1541, 3, 16, 1, True, False), (512, 128, 1541, 3, 16, 2, True, True),
    (512, 100, 1541, 1, 1, 1, True, True), (512, 100, 1541, 3, 128, 2, False, False), (512, 128, 512, 3, 1, 2, True, False),
    (512, 128, 2944, 3, 16, 1, True, True),
    (2048, 512, 2048, 1, 16, 2, True, False), (2048, 512, 6149, 3, 16, 1, True, False), (2048, 512, 6149, 3, 128, 2, True, True),
    (2048, 300, 6149, 1, 16, 1, False, True), (2048, 512, 6149, 1, 1, 1, True, False), (2048, 512, 2048, 3, 16, 1, False, True),
    (2048, 512, 12288, 1, 16, 2, True, True),
]

_REF = {}


def _reference(case):
    """(x, dmel, mel, dx) in float64 on the CPU, computed once per case and shared; white noise (the power 1 cases rely on it:
    no bin of the float64 spectrum lies within 1e-6 of zero relative to the row's peak -- asserted -- or the gradient of |S|
    would be ill-conditioned in any precision)."""
    if case not in _REF:
        n_fft, hop, t, rows, n_mels, power, normalized, center = case
        x = R.white_noise((rows, t), 31 + n_fft + t + n_mels, torch.float64).requires_grad_(True)
        if power == 1:
            assert R.smallest_relative_bin(x.detach(), n_fft, hop, normalized, center) > 1e-6
        mel = R.mel_spectrogram(x, SR, n_fft, hop, n_mels, power, normalized, center)
        g = R.white_noise(tuple(mel.shape), 32 + n_fft + t, torch.float64)
        (dx,) = torch.autograd.grad(mel, x, g)
        _REF[case] = (x.detach(), g, mel.detach(), dx)
    return _REF[case]


def _module(case, dev):
    from rave_amd.mel import DifferentiableMelSpectrogram
    n_fft, hop, t, rows, n_mels, power, normalized, center = case
    return DifferentiableMelSpectrogram(SR, n_fft, hop_length=hop, n_mels=n_mels, power=power, normalized=normalized, center=center).to(dev)


def _covered(case):
    """Samples of an uncentred row that some frame covers."""
    n_fft, hop, t = case[:3]
    return ((t - n_fft) // hop) * hop + n_fft


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_forward_and_backward_against_float64(dev, case):
    from rave_amd import ops
    n_fft, hop, t, rows, n_mels, power, normalized, center = case
    assert ops.mel_diff_supported(n_fft, hop, n_mels, t, rows, center, power)
    x, g, mel, dx = _reference(case)
    m = _module(case, dev)
    xg = x.float().to(dev).requires_grad_(True)
    got = m(xg)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(mel.shape)
    assert got.grad_fn is not None and "MelDiff" in type(got.grad_fn).__name__               # the kernels, not the composition
    nz = mel.abs().sum((0, 2)) > 0                  # (a filter narrower than the bin spacing is all zero in both)
    assert torch.equal(got.detach().cpu().abs().sum((0, 2)) > 0, nz) and bool(nz.any())
    ef, chan = rel_l2(got[:, nz], mel[:, nz]), _per_channel(got[:, nz], mel[:, nz])
    (dxg,) = torch.autograd.grad(got, xg, g.float().to(dev))
    eb = rel_l2(dxg, dx)
    print(f"mel_diff {case}: forward {ef:.2e} overall, worst mel channel {float(chan.max()):.2e}; backward {eb:.2e}")
    assert ef <= BAR and float(chan.max()) <= BAR
    assert bool(torch.isfinite(dxg).all()) and eb <= BAR
    if not center and _covered(case) < t:           # the tail no frame covers: exactly zero, as in the reference
        assert float(dx[:, _covered(case):].abs().max()) == 0.0
        assert bool((dxg[:, _covered(case):] == 0).all())


def test_a_silent_row_gives_zeros_and_no_nan(dev):
    """power 1: d|S| at S = 0 is 0 (torch's abs), not 0 / 0."""
    for case in ((512, 128, 1541, 3, 16, 1, True, False), (2048, 512, 6149, 3, 16, 1, True, True)):
        x, g, mel, dx = _reference(case)
        xs = x.float().clone()
        xs[1] = 0.0
        xg = xs.to(dev).requires_grad_(True)
        got = _module(case, dev)(xg)
        (dxg,) = torch.autograd.grad(got, xg, g.float().to(dev))
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dxg).all())
        assert bool((got[1] == 0).all()) and bool((dxg[1] == 0).all())
        assert rel_l2(dxg[0], dx[0]) <= BAR and rel_l2(dxg[2], dx[2]) <= BAR            # the neighbours are what they were


@pytest.mark.parametrize("case", [(128, 32, 5000, 3, 16, 1, True, False), (512, 100, 1541, 3, 128, 2, False, False),
                                  (2048, 512, 6149, 3, 128, 2, True, True)], ids=str)
def test_two_runs_give_the_same_bits(dev, case):
    x, g, mel, dx = _reference(case)
    m = _module(case, dev)
    xg, gg = x.float().to(dev).requires_grad_(True), g.float().to(dev)
    runs = []
    for _ in range(2):
        out = m(xg)
        runs.append((out.detach().clone(), torch.autograd.grad(out, xg, gg)[0].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("case", [(128, 32, 389, 3, 16, 1, True, True), (512, 128, 1541, 3, 16, 1, True, False),
                                  (2048, 512, 6149, 3, 128, 2, True, True)], ids=str)
def test_pointers_that_are_only_4_byte_aligned(dev, case):
    import misaligned as MA
    from rave_amd import _lib as L, ops
    n_fft, hop, t, rows, n_mels, power, normalized, center = case
    xr, g, mel, dx = _reference(case)
    m = _module(case, dev)
    bins, scale = m._device_tables(dev)
    x, gg, w, fb = xr.float().to(dev), g.float().to(dev), m.spectrogram.window, m.mel_scale.fb
    tw = ops._twiddle(n_fft, dev)

    def fwd(xv, wv, fv, bv, out):
        return L.lib.rh_mel_diff_fwd_f32(L.ptr(xv), L.ptr(wv), L.ptr(tw), L.ptr(fv), L.ptr(bv), rows, t, n_fft, hop, n_mels, int(center),
                                         power, scale, L.ptr(out), L.stream())

    def bwd(gv, xv, wv, fv, bv, out):
        return L.lib.rh_mel_diff_bwd_f32(L.ptr(gv), L.ptr(xv), L.ptr(wv), L.ptr(tw), L.ptr(fv), L.ptr(bv), rows, t, n_fft, hop, n_mels,
                                         int(center), power, scale, L.ptr(out), L.stream())

    base_o, base_d = torch.zeros_like(gg), torch.zeros_like(x)
    assert all(v.data_ptr() % 16 == 0 for v in (x, gg, base_o, base_d))
    assert fwd(x, w, fb, bins, base_o) == 0 and bwd(gg, x, w, fb, bins, base_d) == 0
    for off in (1, 2, 3):
        xs, ws, fs, gs = MA.carve(x, off), MA.carve(w, (off + 1) % 4), MA.carve(fb, (off + 2) % 4), MA.carve(gg, off)
        bs = MA.carve(bins, (off + 3) % 4)
        os_, ds = MA.carve(torch.zeros_like(gg), (off + 2) % 4 or 1), MA.carve(torch.zeros_like(x), off)
        assert fwd(xs, ws, fs, bs, os_) == 0 and bwd(gs, xs, ws, fs, bs, ds) == 0
        torch.cuda.synchronize()
        assert torch.equal(os_, base_o) and torch.equal(ds, base_d), off
        assert all(MA.guards_intact(v) for v in (xs, ws, fs, gs, bs, os_, ds)), off


def _loss(scales=(256, 512), power=1):
    from rave_amd.losses import EncodecAudioDistance, SpectralDistance
    return EncodecAudioDistance(list(scales), partial(SpectralDistance, sampling_rate=SR, norm=("L1", "L2"), power=power, normalized=True,
                                                      mel=16))


def test_recorded_loss_equals_the_eager_one(dev):
    m = _loss().to(dev)
    x = R.white_noise((2, 1, 4096), 41).to(dev)
    y = R.white_noise((2, 1, 4096), 42).to(dev).requires_grad_(True)

    def step():
        out = m(x, y)
        total = out["waveform_distance"] + out["spectral_distance"]
        return total, torch.autograd.grad(total, y)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]                        # the eager call: tables and twiddles are made here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, gy = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(total.detach(), eager[0]) and torch.equal(gy, eager[1])
    assert float(eager[0]) > 0 and float(eager[1].abs().max()) > 0


def test_first_call_inside_a_capture_raises(dev):
    from rave_amd import ops
    from rave_amd.mel import DifferentiableMelSpectrogram
    ops._twiddle(256, dev)                                                  # (so that it is the module's own check that speaks)
    m = DifferentiableMelSpectrogram(SR, 256, hop_length=64, n_mels=16, power=1, center=False).to(dev)
    x = R.white_noise((2, 1024), 43).to(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="first call inside a hipGraph capture"):
        with torch.cuda.graph(graph):
            m(x)
    torch.cuda.synchronize()
    assert tuple(m(x).shape) == (2, 16, 13)                                 # and eagerly it runs


@pytest.mark.parametrize("power", [1, 2])
def test_encodec_distance_end_to_end(dev, power):
    """Both dictionary entries and grad_y of EncodecAudioDistance on the mel variant against the float64 restatement at the 1e-5
    tests/test_oracle.py holds the plain variant to."""
    m = _loss(power=power).to(dev)
    x, y = R.white_noise((2, 1, 4096), 44), R.white_noise((2, 1, 4096), 45)
    yg = y.to(dev).requires_grad_(True)
    got = m(x.to(dev), yg)
    (gy,) = torch.autograd.grad(got["waveform_distance"] + got["spectral_distance"], yg)
    y64 = y.double().requires_grad_(True)
    want = R.encodec_audio_distance(x.double(), y64, [256, 512], SR, ("L1", "L2"), power, True, 16)
    (gy64,) = torch.autograd.grad(want["waveform_distance"] + want["spectral_distance"], y64)
    for k in ("waveform_distance", "spectral_distance"):
        e = abs(float(got[k].detach()) - float(want[k].detach())) / abs(float(want[k].detach()))
        print(f"encodec mel distance, power {power}: {k} off by {e:.2e}")
        assert e <= 1e-5, k
    print(f"encodec mel distance, power {power}: grad_y rel L2 {rel_l2(gy, gy64):.2e}")
    assert rel_l2(gy, gy64) <= 1e-5
