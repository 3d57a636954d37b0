"""CPU tests of the mel-spectrogram encoder input (rave/model.py:238-242, configs/hybrid.gin): the test-side reference
(tests/mel_reference.py) reproduces the filterbank facts it was written against, ``rave_amd.MelSpectrogram`` carries torchaudio's
buffers and agrees with it on the CPU, ``build_v2(mel_input=True)`` loads a reference-shaped checkpoint, and the C entry points
refuse what they do not build before anything touches a GPU."""
import os
import re

import pytest
import torch

import mel_reference as R

RH_ERR_INVALID, RH_ERR_UNSUPPORTED = -1, -2
HYBRID = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=256, normalized=True, n_mels=128)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "mel_tiny.pt"), weights_only=False)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def test_filterbank_facts():
    """melscale_fbanks(f_min=0, f_max=sr // 2, htk, norm=None) in float64: shapes, sums and supports as computed when the
    helper was written; the float32 filterbank (torchaudio's own precision) is the same to float32 rounding."""
    def fb(sr, n_fft, n_mels, dtype=torch.float64):
        return R.melscale_fbanks(n_fft // 2 + 1, 0.0, float(sr // 2), n_mels, sr, dtype=dtype)
    a = fb(44100, 2048, 128)
    assert tuple(a.shape) == (1025, 128)
    assert abs(float(a.sum()) - 1009.432974312) < 1e-8
    assert float(a[0].abs().max()) == 0.0
    assert float(a[-1].abs().max()) < 1e-14
    per_filter = (a != 0).sum(0)
    assert (int(per_filter.min()), int(per_filter.max())) == (1, 56)
    assert int((a != 0).sum(1).max()) <= 2
    b = fb(48000, 2048, 128)
    assert tuple(b.shape) == (1025, 128) and abs(float(b.sum()) - 1009.139713442) < 1e-8
    c = fb(44100, 256, 16)
    assert tuple(c.shape) == (129, 16) and abs(float(c.sum()) - 115.267668111) < 1e-8
    per_filter = (c != 0).sum(0)
    assert (int(per_filter.min()), int(per_filter.max())) == (2, 45)
    for sr, n_fft, n_mels, ref in ((44100, 2048, 128, a), (48000, 2048, 128, b), (44100, 256, 16, c)):
        f32 = fb(sr, n_fft, n_mels, torch.float32)
        assert f32.dtype == torch.float32 and float((f32.double() - ref).abs().max()) < 2e-5
        assert int((f32 != 0).sum(1).max()) <= 2


@pytest.mark.parametrize("shape,amp,bound", [((2, 1, 4096), 1.0, 1e-6), ((3, 2, 4096), 1.0, 1e-6), ((2, 1, 4096), 1e-3, 1e-6),
                                             ((3, 2, 4096), 1e-3, 1e-6), ((2, 1, 1280), 1.0, 1e-6), ((2, 1, 4196), 1.0, 1e-6)])
def test_helper_float32_agrees_with_float64(shape, amp, bound):
    """float32 rounding of a 2048-point transform and of sums of <= 56 products: of the order of 1e-7 (1e-6 is 10 x that)."""
    x = R.white_noise(shape, amp, 1)
    m = R.MelSpectrogram(**HYBRID)
    y32 = R.log_mel(m, x)
    y64 = R.log_mel(R.MelSpectrogram(**HYBRID).double(), x.double())
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert tuple(y32.shape) == (shape[0], shape[1] * 128, shape[2] // 256)
    assert _rel(y32, y64) < bound


def test_helper_against_torchaudio_where_it_is_installed():
    """Only where a real torchaudio with a working MelSpectrogram imports (it is not a dependency of this project)."""
    try:
        from torchaudio.transforms import MelSpectrogram as TA
        ta = TA(**HYBRID)
    except Exception as e:                               # noqa: BLE001 -- not installed, or a stub whose constructor raises
        pytest.skip(f"no working torchaudio.transforms.MelSpectrogram here ({type(e).__name__})")
    ref = R.MelSpectrogram(**HYBRID)
    assert sorted((k, tuple(v.shape)) for k, v in ta.state_dict().items()) == sorted((k, tuple(v.shape)) for k, v in ref.state_dict().items())
    for k, v in ta.state_dict().items():
        assert float((ref.state_dict()[k] - v).abs().max()) < 1e-6, k
    x = R.white_noise((2, 1, 4096), 1.0, 1)
    assert _rel(ref(x), ta(x)) < 1e-5


def test_helper_float32_meets_the_onset_bound():
    """Frames that lie wholly in the quiet half keep their own precision next to the loud half (separate transforms)."""
    x = R.onset()
    y32 = R.log_mel(R.MelSpectrogram(**HYBRID), x)
    y64 = R.log_mel(R.MelSpectrogram(**HYBRID).double(), x.double())
    quiet = [f for f in range(y64.shape[-1]) if f * 256 + 1024 <= 4096]
    assert len(quiet) >= 10
    for f in quiet:
        assert _rel(y32[..., f], y64[..., f]) <= 1e-4, f


def test_module_against_the_helper_on_the_cpu(fixture):
    import rave_amd
    from rave_amd.mel import MelSpectrogram
    assert rave_amd.MelSpectrogram is MelSpectrogram
    ours, ref = MelSpectrogram(**HYBRID), R.MelSpectrogram(**HYBRID)
    got = sorted((k, tuple(v.shape)) for k, v in ours.state_dict().items())
    assert got == [(k, tuple(s)) for k, s in fixture["spectrogram_keys"]]
    assert got == [("mel_scale.fb", (1025, 128)), ("spectrogram.window", (2048,))]
    for k, v in ref.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    ours.load_state_dict(ref.state_dict(), strict=True)
    x = fixture["x"]
    full = ours(x)
    assert tuple(full.shape) == (2, 1, 128, 17) and not full.requires_grad
    assert _rel(full, ref.double()(x.double())) < 1e-6
    lm = ours.log_mel(x.clone().requires_grad_(True))
    assert tuple(lm.shape) == (2, 1, 128, 16) and not lm.requires_grad
    assert _rel(lm.reshape(2, 128, 16), fixture["mel"]) < 1e-6
    small = MelSpectrogram(sample_rate=44100, n_fft=256, hop_length=32, n_mels=16)
    assert _rel(small(x), R.MelSpectrogram(sample_rate=44100, n_fft=256, hop_length=32, n_mels=16).double()(x.double())) < 1e-6


def test_unbuilt_arguments_raise():
    from rave_amd.mel import MelSpectrogram
    for bad in (dict(power=1.0), dict(power=None), dict(center=False), dict(pad_mode="constant"), dict(mel_scale="slaney"),
                dict(norm="slaney"), dict(win_length=1024), dict(pad=8), dict(window_fn=torch.hamming_window), dict(onesided=False)):
        with pytest.raises(NotImplementedError):
            MelSpectrogram(**{**HYBRID, **bad})


def test_raw_modes_raise_and_defaults_are_unchanged():
    from rave_amd import model as M
    kw = dict(capacity=16, latent_size=16, disc_capacity=16)
    torch.manual_seed(0)
    base = M.build_v2(**kw)
    torch.manual_seed(0)
    off = M.build_v2(mel_input=False, **kw)
    assert list(base.state_dict()) == list(off.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(base.state_dict().values(), off.state_dict().values()))
    assert base.input_mode == "pqmf" and base.output_mode == "pqmf" and base.spectrogram is None
    assert not any("spectrogram" in k for k in base.state_dict())

    import inspect
    args = dict(latent_size=16, sampling_rate=44100, encoder=None, decoder=None, discriminator=None, phase_1_duration=1,
                gan_loss=None, valid_signal_crop=False, feature_matching_fun=None, num_skipped_features=0, audio_distance=None,
                multiband_audio_distance=None)
    assert {"spectrogram", "input_mode", "output_mode"} <= set(inspect.signature(M.RAVE.__init__).parameters)
    for bad in (dict(input_mode="raw"), dict(output_mode="raw"), dict(input_mode="raw", output_mode="raw")):
        with pytest.raises(NotImplementedError, match="raw"):
            M.RAVE(**args, **bad)
    with pytest.raises(ValueError):
        M.RAVE(**args, input_mode="mel")                     # no spectrogram
    with pytest.raises(ValueError):
        M.RAVE(**args, input_mode="stft")


def test_reference_shaped_checkpoint_loads_strictly(fixture):
    """The golden's encoder state_dict is the reference's (EncoderV2(data_size=128, ratios=[2, 2, 2], dilations=[1])), the
    spectrogram keys are torchaudio's: together with the rest of the model they load with strict=True."""
    from rave_amd import model as M
    m = M.build_v2(mel_input=True, gru_layers=2, capacity=fixture["capacity"], latent_size=fixture["latent_size"], disc_capacity=16)
    assert m.input_mode == "mel"
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    enc_keys = [k for k in sd if k.startswith("encoder.")]
    assert sorted(k[len("encoder."):] for k in enc_keys) == sorted(fixture["state_dict"])
    for k, v in fixture["state_dict"].items():
        assert sd["encoder." + k].shape == v.shape, k
        sd["encoder." + k] = v.clone()
    ref = R.MelSpectrogram(**HYBRID)
    assert sorted(k for k in sd if k.startswith("spectrogram.")) == ["spectrogram.mel_scale.fb", "spectrogram.spectrogram.window"]
    for k, v in ref.state_dict().items():
        sd["spectrogram." + k] = v.clone()
    m.load_state_dict(sd, strict=True)
    assert m.encoder.encoder.net[0].weight_v.shape == (fixture["capacity"], 128, 7)
    stereo = M.build_v2(mel_input=True, n_channels=2, capacity=16, latent_size=16, disc_capacity=16)
    assert stereo.encoder.encoder.net[0].weight_v.shape == (16, 256, 7)       # data_size * n_channels, as the reference


def test_mismatched_latent_rates_are_refused():
    from rave_amd import model as M
    with pytest.raises(ValueError, match="2048.*1024"):
        M.build_v2(mel_input=True, ratios=(4, 4, 2, 2), capacity=16, latent_size=16, disc_capacity=16)
    with pytest.raises(ValueError):
        M.build_v2(mel_input=True, hop_length=512, capacity=16, latent_size=16, disc_capacity=16)


def test_cpu_encode_follows_the_raw_audio_for_the_multiband_signal(fixture):
    """encode(return_mb=True) in mel mode: the PQMF of the RAW audio, not of the mel tensor (the reference's defect)."""
    from rave_amd import model as M
    m = M.build_v2(mel_input=True, capacity=16, latent_size=16, disc_capacity=16)
    x = fixture["x"]
    mel = m._mel_encode(x.clone().requires_grad_(True))
    assert tuple(mel.shape) == (2, 128, 16) and not mel.requires_grad
    assert _rel(mel, fixture["mel"]) < 1e-6


def test_entry_points_answer_for_built_and_unbuilt_sizes():
    from rave_amd import _lib as L
    lib = L.lib
    for n_fft, hop, n_mels, t, rows, want in (
            (2048, 256, 128, 65536, 32, 1), (2048, 256, 128, 1025, 1, 1), (256, 32, 16, 4096, 6, 1), (128, 128, 1, 128, 1, 1),
            (512, 100, 80, 1000, 3, 1), (1024, 256, 128, 4096, 65535, 1),
            (2048, 256, 128, 1024, 1, 0),            # T must exceed n_fft / 2 (reflect padding)
            (4096, 256, 128, 65536, 1, 0), (64, 16, 16, 4096, 1, 0), (1000, 250, 64, 4096, 1, 0), (2048, 0, 128, 4096, 1, 0),
            (2048, -256, 128, 4096, 1, 0), (2048, 4096, 128, 8192, 1, 0), (2048, 256, 129, 4096, 1, 0), (2048, 256, 0, 4096, 1, 0),
            (2048, 256, 128, 4096, 0, 0), (2048, 256, 128, 4096, 65536, 0), (2048, 256, 128, 2 ** 31 - 1, 1, 0)):
        assert lib.rh_mel_supported(n_fft, hop, n_mels, t, rows) == want, (n_fft, hop, n_mels, t, rows)

    p = 64               # never dereferenced: every call below is refused before a launch

    def fwd(x=p, win=p, tw=p, fb=p, bins=p, rows=2, t=4096, n_fft=2048, hop=256, n_mels=128, n_frames=16, scale=1.0, y=p):
        return lib.rh_mel_fwd_f32(x, win, tw, fb, bins, rows, t, n_fft, hop, n_mels, n_frames, scale, 1, y, None)

    for name in ("x", "win", "tw", "fb", "bins", "y"):
        assert fwd(**{name: None}) == RH_ERR_INVALID, name
        assert b"null" in lib.rh_last_error()
    for bad in (dict(n_fft=4096), dict(n_fft=1000), dict(hop=0), dict(hop=4096), dict(n_mels=129), dict(n_mels=0), dict(t=1024),
                dict(rows=0), dict(rows=65536)):
        assert fwd(**bad) == RH_ERR_UNSUPPORTED, bad
        assert lib.rh_last_error()
    assert b"4096" in (fwd(n_fft=4096), lib.rh_last_error())[1]
    assert fwd(n_frames=15) == RH_ERR_INVALID and fwd(n_frames=18) == RH_ERR_INVALID
    assert fwd(tw=68) == RH_ERR_INVALID and b"aligned" in lib.rh_last_error()
    assert fwd(scale=0.0) == RH_ERR_INVALID and fwd(scale=float("nan")) == RH_ERR_INVALID and fwd(scale=float("inf")) == RH_ERR_INVALID


def test_hybrid_overlay_binds_what_hybrid_gin_binds():
    """rave_amd/configs/mi355x_hybrid.gin carries configs/hybrid.gin's bindings for the drop-in classes, both halves."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rave_amd", "configs", "mi355x_hybrid.gin")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    assert re.search(r"^N_FFT = 2048\s*$", code, re.M) and re.search(r"^N_MELS = 128\s*$", code, re.M)
    assert re.search(r"^HOP_LENGTH = 256\s*$", code, re.M) and re.search(r"^ENCODER_RATIOS = \[2, 2, 2\]\s*$", code, re.M)
    assert re.search(r"rave_amd\.blocks\.EncoderV2:\s*\n\s+data_size = %N_MELS\s*\n\s+ratios = %ENCODER_RATIOS\s*\n\s+dilations = \[1\]\s*\n", code)
    assert re.search(r"rave_amd\.mel\.MelSpectrogram:\s*\n\s+sample_rate = %SAMPLING_RATE\s*\n\s+n_fft = %N_FFT\s*\n\s+win_length = %N_FFT\s*\n"
                     r"\s+hop_length = %HOP_LENGTH\s*\n\s+normalized = True\s*\n\s+n_mels = %N_MELS\s*\n", code)
    assert re.search(r"rave_amd\.blocks\.GeneratorV2:\s*\n\s+recurrent_layer = @rave_amd\.blocks\.GRU\s*\n", code)
    assert re.search(r"rave_amd\.blocks\.GRU:\s*\n\s+latent_size = %LATENT_SIZE\s*\n\s+num_layers = %NUM_GRU_LAYERS\s*\n", code)
    assert re.search(r"^NUM_GRU_LAYERS = 2\s*$", code, re.M)
    assert re.search(r"core\.n_fft_to_num_bands:\s*\n\s+n_fft = %N_FFT\s*\n", code)
    assert re.search(r"rave\.RAVE:\s*\n\s+spectrogram = @rave_amd\.mel\.MelSpectrogram\(\)\s*\n\s+input_mode = \"mel\"\s*(\n|$)", code)
    assert "import rave_amd.mel" in code and "import rave_amd.blocks" in code
    assert "raw" in text.lower()                         # the header says which modes remain unbuilt
