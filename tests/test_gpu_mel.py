"""GPU tests of the mel-spectrogram encoder input (rave_amd/csrc/mel.hip, rave_amd.mel.MelSpectrogram, RAVE.input_mode =
"mel"): the kernel against the float64 reference of tests/mel_reference.py at the project's parity bar (relative L2 <= 1e-4,
overall AND per mel channel), layout / reflect / onset cases, misaligned pointers, repeatability, refusals, the golden of the
unmodified reference, and one training step eager vs recorded.

For scale: the float32 torch composition differs from float64 by 6.6e-8 (white noise at amplitude 1) and 1.6e-7 (at 1e-3)."""
import ctypes as C
import os

import pytest
import torch

import mel_reference as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

BAR = 1e-4
HYBRID = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=256, normalized=True, n_mels=128)
RH_ERR_INVALID, RH_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref64():
    return R.MelSpectrogram(**HYBRID).double()


@pytest.fixture(scope="module")
def ours(dev):
    from rave_amd.mel import MelSpectrogram
    return MelSpectrogram(**HYBRID).to(dev)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "mel_tiny.pt"), weights_only=False)


def _per_channel(got, want):
    """Relative L2 of every mel channel over all rows and frames: (..., n_mels, frames) -> n_mels values."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    g, w = g.reshape(-1, *g.shape[-2:]), w.reshape(-1, *w.shape[-2:])
    return (g - w).pow(2).sum((0, 2)).sqrt() / w.pow(2).sum((0, 2)).sqrt()


def _check(tag, got, want):
    total, chan = rel_l2(got, want), _per_channel(got, want)
    print(f"mel {tag}: rel L2 {total:.2e} overall, worst mel channel {float(chan.max()):.2e} (channel {int(chan.argmax())})")
    assert tuple(got.shape) == tuple(want.shape)
    assert total <= BAR
    assert float(chan.max()) <= BAR, int(chan.argmax())


@pytest.mark.parametrize("shape,amp", [((2, 1, 4096), 1.0), ((3, 2, 4096), 1.0), ((2, 1, 4096), 1e-3), ((3, 2, 4096), 1e-3),
                                       ((2, 1, 1280), 1.0),      # every frame reflects at one or both ends
                                       ((2, 1, 4196), 1.0)])     # not a multiple of the hop
def test_white_noise_against_float64(dev, ours, ref64, shape, amp):
    x = R.white_noise(shape, amp, 3)
    want = torch.log1p(ref64(x.double())[..., :-1])
    got = ours.log_mel(x.to(dev))
    assert got.dtype == torch.float32 and not got.requires_grad
    assert tuple(got.shape) == (shape[0], shape[1], 128, shape[2] // 256)
    _check(f"{shape} x {amp:g}", got, want)


def test_forward_is_torchaudios_result(dev, ours, ref64):
    """forward(): all T // hop + 1 frames of the power mel spectrogram, no logarithm."""
    x = R.white_noise((3, 2, 4196), 1.0, 4)
    got = ours(x.to(dev))
    assert tuple(got.shape) == (3, 2, 128, 17)
    _check("forward (3, 2, 4196)", got, ref64(x.double()))


def test_tones_peak_in_the_reference_channel(dev, ours, ref64):
    bins = [37, 200, 517, 900]
    x = R.tones(2048, 4096, bins)
    want = torch.log1p(ref64(x.double())[..., :-1])
    got = ours.log_mel(x.to(dev)).cpu()
    interior = [f for f in range(16) if f * 256 - 1024 >= 0 and f * 256 + 1024 <= 4096]
    assert len(interior) >= 5
    peaks = want[..., interior].argmax(-2)
    assert len({int(p) for p in peaks[:, 0, 0]}) == len(bins)            # the rows peak in different channels
    assert torch.equal(got[..., interior].argmax(-2), peaks)
    # (overall only: far from the tone the float64 value is window leakage below float32's rounding of the peak)
    print(f"mel tones: rel L2 {rel_l2(got, want):.2e} overall")
    assert rel_l2(got, want) <= BAR


def test_onset_quiet_frames_keep_their_precision(dev, ours, ref64):
    """8192 samples, 1e-4 then 1: every frame whose window lies wholly in the quiet half, each on its own.  A pair transform
    that lets the loud frame's rounding leak into its quiet partner misses this by an order of magnitude."""
    x = R.onset()
    want = torch.log1p(ref64(x.double())[..., :-1])
    cpu32 = torch.log1p(R.MelSpectrogram(**HYBRID)(x)[..., :-1])
    got = ours.log_mel(x.to(dev))
    quiet = [f for f in range(want.shape[-1]) if f * 256 + 1024 <= 4096]
    assert len(quiet) >= 10
    worst = 0.0
    for f in quiet:
        assert rel_l2(cpu32[..., f], want[..., f]) <= BAR, f              # the float32 reference meets it ...
        e = rel_l2(got[..., f], want[..., f])
        worst = max(worst, e)
        assert e <= BAR, (f, e)                                           # ... and so does the kernel
    print(f"mel onset: worst quiet frame rel L2 {worst:.2e}")


@pytest.mark.parametrize("n_fft,hop,n_mels,t", [(128, 16, 16, 1000), (256, 32, 16, 1000), (256, 100, 40, 777), (512, 128, 64, 2000),
                                                (1024, 256, 128, 3000)])
def test_the_other_built_sizes(dev, n_fft, hop, n_mels, t):
    from rave_amd.mel import MelSpectrogram
    kw = dict(sample_rate=44100, n_fft=n_fft, hop_length=hop, n_mels=n_mels, normalized=True)
    x = R.white_noise((3, 2, t), 1.0, 6)
    want = torch.log1p(R.MelSpectrogram(**kw).double()(x.double())[..., :-1])
    got = MelSpectrogram(**kw).to(dev).log_mel(x.to(dev))
    nz = want.abs().sum((0, 1, 3)) > 0              # (a filter narrower than the bin spacing is all zero in both)
    assert torch.equal(got.cpu().abs().sum((0, 1, 3)) > 0, nz)
    _check(f"n_fft {n_fft} hop {hop} n_mels {n_mels}", got[:, :, nz], want[:, :, nz])


def _raw_call(L, x, win, tw, fb, bins, y, n_fft=2048, hop=256, n_mels=128, scale=1.0):
    rows, t = x.shape[0] * x.shape[1], x.shape[-1]
    return L.lib.rh_mel_fwd_f32(L.ptr(x), L.ptr(win), L.ptr(tw), L.ptr(fb), L.ptr(bins), rows, t, n_fft, hop, n_mels, t // max(hop, 1), scale, 1,
                                L.ptr(y), L.stream())


def test_pointers_that_are_only_4_byte_aligned(dev, ours):
    import misaligned as MA
    from rave_amd import _lib as L, ops
    x = R.white_noise((3, 2, 4196), 1.0, 7).to(dev)
    bins, scale = ours._device_tables(dev)
    base = ours.log_mel(x)
    xs, ws, fs = MA.carve(x, 1), MA.carve(ours.spectrogram.window, 3), MA.carve(ours.mel_scale.fb, 2)
    bs = MA.carve(bins, 1)
    ys = MA.carve(torch.zeros_like(base), 3)
    assert _raw_call(L, xs, ws, ops._twiddle(2048, dev), fs, bs, ys, scale=scale) == 0
    torch.cuda.synchronize()
    assert torch.equal(ys, base)
    assert MA.guards_intact(ys) and MA.guards_intact(xs)


def test_two_launches_give_the_same_bits(dev, ours):
    x = R.white_noise((3, 2, 4196), 1.0, 8).to(dev)
    a = ours.log_mel(x)
    b = ours.log_mel(x)
    assert torch.equal(a, b)


def test_unbuilt_geometry_is_refused_and_writes_nothing(dev, ours):
    import misaligned as MA
    from rave_amd import _lib as L, ops
    x = R.white_noise((2, 1, 8192), 1.0, 9).to(dev)
    bins, scale = ours._device_tables(dev)
    y = torch.empty(2, 1, 128, 64, device=dev)
    MA.fill_guard(y)
    tw = ops._twiddle(2048, dev)
    args = (x, ours.spectrogram.window, tw, ours.mel_scale.fb, bins, y)
    for bad in (dict(n_fft=4096), dict(n_fft=1000), dict(hop=0), dict(hop=4096), dict(n_mels=129)):
        assert _raw_call(L, *args, **{**dict(scale=scale), **bad}) == RH_ERR_UNSUPPORTED, bad
    short = x[..., :1024].contiguous()
    assert _raw_call(L, short, *args[1:], scale=scale) == RH_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert MA.is_guard(y)
    with pytest.raises(NotImplementedError):
        ours.log_mel(short)


def test_golden_mel_and_encoder(dev, ours, fixture):
    """The unmodified reference's ``_mel_encode`` and mel-sized encoder (tools/make_golden_mel.py): the kernel's mel, then the
    drop-in encoder ON the kernel's mel -- output at the end-to-end bar, parameter gradients at the 2e-4 of the encoder parity
    tests, plus what the counted LeakyReLU gate flips downstream of a tensor account for (none without a flip)."""
    from gate_flips import chain_flips, flip_allowance_by_param, name_gate_log
    from rave_amd import model as M, ops
    g = fixture
    x = g["x"].to(dev)
    m = M.build_v2(mel_input=True, capacity=g["capacity"], latent_size=g["latent_size"], disc_capacity=16)
    m.encoder.load_state_dict(g["state_dict"], strict=True)
    m = m.to(dev).train()
    mel = m._mel_encode(x)
    print(f"mel golden: kernel vs recorded float32 mel rel L2 {rel_l2(mel, g['mel']):.2e}")
    assert tuple(mel.shape) == tuple(g["mel"].shape) and rel_l2(mel, g["mel"]) <= BAR
    ops.gate_log_begin()
    z = m.encoder(mel)
    log = name_gate_log(ops.gate_log_end(), m.encoder)
    assert rel_l2(z, g["z"]) <= BAR, rel_l2(z, g["z"])
    z.backward(g["dz"].to(dev))
    flips, n_gates, _ = chain_flips(log, g["gates"])
    allow = flip_allowance_by_param(log, flips)
    named = dict(m.encoder.named_parameters())
    worst = 0.0
    for k, gref in g["grads"].items():
        assert named[k].grad is not None, k
        e = rel_l2(named[k].grad, gref)
        worst = max(worst, e)
        assert e < min(2e-4 + 3.0 * allow.get(k, 0.0), 1e-2), (k, e, allow.get(k, 0.0))
    print(f"mel golden: encoder z rel L2 {rel_l2(z, g['z']):.2e}, worst gradient {worst:.2e}, {sum(flips)} of {n_gates} gates flipped")


# ---- one training step of the shrunk hybrid model ---------------------------------------------------------------------------
# 18432 samples = 9 latent frames: the 2048-point scale of the multiband distance reflect-pads its input by 1024 band samples, so a
# clip must have more than 16 x 1024 samples -- on the reference as well; the next multiple of the latent rate (2048) is used.
KW = dict(mel_input=True, gru_layers=2, capacity=16, latent_size=16, disc_capacity=16)
N, STEPS = 18432, 3


def _train(dev, graphed):
    from rave_amd import model as M
    torch.manual_seed(0)
    m = M.build_v2(**KW).to(dev).train()
    m.configure_optimizers(capturable=True)
    xs = [R.white_noise((2, 1, N), 0.1, 70 + i).to(dev) for i in range(STEPS)]
    gen = torch.Generator().manual_seed(2)
    es = [torch.randn(2, 16, N // 2048, generator=gen).to(dev) for _ in range(STEPS)]
    step = M.GraphedTrainingStep(m, xs[0], inject_eps=True) if graphed else None
    losses = []
    for i in range(STEPS):
        logged = step(xs[i], i, eps=es[i]) if graphed else m.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
        losses.append({k: torch.as_tensor(v).detach().clone() for k, v in logged.items()})
        m.on_train_batch_end(None, None, i)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in m.named_parameters()}, losses


def test_step_eager_and_recorded_are_bit_identical(dev):
    pe, le = _train(dev, False)
    pg, lg = _train(dev, True)
    for a, b in zip(le, lg):
        assert sorted(a) == sorted(b)
        for k in a:
            assert bool(torch.isfinite(a[k]).all()), k
            assert torch.equal(a[k], b[k]), k
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    assert any(not torch.equal(v, torch.zeros_like(v)) for v in le[0].values())


def test_step_feeds_the_multiband_distance_the_raw_audio_and_skips_the_first_data_gradient(dev):
    from rave_amd import model as M, ops
    torch.manual_seed(0)
    m = M.build_v2(**KW).to(dev).train()
    m.configure_optimizers()
    x = R.white_noise((2, 1, N), 0.1, 70).to(dev)
    eps = torch.randn(2, 16, N // 2048, generator=torch.Generator().manual_seed(2)).to(dev)
    seen = []
    hook = m.multiband_audio_distance.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    ops.plan_log_begin()
    logged = m.training_step(x.clone(), 0, eps=eps)
    plans = ops.plan_log_end()
    hook.remove()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logged.values())
    with torch.no_grad():
        want = M._pqmf_encode(m.pqmf, x)
    assert len(seen) == 1 and tuple(seen[0].shape) == (2, 16, N // 16) and torch.equal(seen[0], want)
    # the encoder's first convolution (128 mel channels in, kernel 7) ran forward and recorded no data-gradient launch
    first = [(which, geo) for which, geo, _ in plans if geo[0] == 128 and geo[2] == 7]
    assert [w for w, _ in first] == [0], first
    assert any(which == 1 for which, _, _ in plans)                      # (the log does see the other data gradients)
    z, x_mb = m.encode(x, return_mb=True)
    assert torch.equal(x_mb, want) and tuple(z.shape) == (2, 32, N // 2048)
