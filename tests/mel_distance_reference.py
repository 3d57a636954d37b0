"""Test-side reference of the mel variant of ``core.SpectralDistance`` / ``core.EncodecAudioDistance`` (rave/core.py:415-490; a
plain helper module, no fixtures): torchaudio is not installed where the tests run, and the oracle's torchaudio shim does not
implement MelSpectrogram, so the yardstick is this restatement of torchaudio's documented computation --
``MelSpectrogram(sr, n_fft, hop_length, n_mels, power, normalized, center)``: periodic Hann window, frames of n_fft samples every
hop (reflect-padded by n_fft / 2 when centred, none otherwise), one-sided spectrum, divided by sqrt(sum(window^2)) when
normalised, ``|.|^power``, ``MelScale(f_min=0, f_max=sr // 2, htk, norm=None)`` -- and of the reference's ``mean_difference``.
Everything runs in the dtype of the input: float64 inputs give the float64 reference, and autograd through it the reference
gradient.  Written apart from rave_amd on purpose: the framing is an explicit pad + unfold + rfft, not torch.stft, the
magnitude is sqrt(re^2 + im^2) of the two planes, and the filterbank comes from tests/mel_reference.py.
"""
import torch

from mel_reference import melscale_fbanks


def filterbank(sample_rate, n_fft, n_mels, dtype=torch.float64):
    """The float32 filterbank torchaudio builds (its own precision), cast to ``dtype``."""
    return melscale_fbanks(n_fft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).to(dtype)


def spectrum(x, n_fft, hop, normalized, center, window=None):
    """(..., T) -> (re, im), each (..., frames, bins), in x's dtype."""
    w = torch.hann_window(n_fft, periodic=True, dtype=x.dtype) if window is None else window.to(x.dtype)
    lead, t = x.shape[:-1], x.shape[-1]
    rows = x.reshape(-1, t)
    if center:
        rows = torch.nn.functional.pad(rows.unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    s = torch.fft.rfft(rows.unfold(-1, n_fft, hop) * w, dim=-1)
    if normalized:
        s = s / w.pow(2).sum().sqrt()
    return s.real.reshape(*lead, *s.shape[-2:]), s.imag.reshape(*lead, *s.shape[-2:])


def mel_spectrogram(x, sample_rate, n_fft, hop, n_mels, power, normalized, center, fb=None, window=None):
    """(..., T) -> (..., n_mels, frames) in x's dtype."""
    re, im = spectrum(x, n_fft, hop, normalized, center, window)
    p = re * re + im * im
    if power == 1:
        p = p.sqrt()
    else:
        assert power == 2
    fb = filterbank(sample_rate, n_fft, n_mels, x.dtype) if fb is None else fb.to(x.dtype)
    return (p @ fb).transpose(-1, -2)


def smallest_relative_bin(x, n_fft, hop, normalized, center):
    """min over the bins of |S| / (the row's largest |S|): the conditioning of d|S| (power 1) on this input."""
    re, im = spectrum(x.double(), n_fft, hop, normalized, center)
    mag = (re * re + im * im).sqrt()
    mag = mag.reshape(-1, mag.shape[-2] * mag.shape[-1])
    return float((mag / mag.max(1, keepdim=True).values).min())


def mean_difference(target, value, norm):
    """rave/core.py:236-252 with relative=False."""
    d = target - value
    if norm == "L1":
        return d.abs().mean()
    assert norm == "L2"
    return (d * d).mean()


def spectral_distance(x, y, n_fft, sample_rate, norms, power, normalized, n_mels):
    """SpectralDistance(n_fft, sample_rate, norms, power, normalized, mel=n_mels)(x, y): hop n_fft / 4, center=False."""
    mx = mel_spectrogram(x, sample_rate, n_fft, n_fft // 4, n_mels, power, normalized, False)
    my = mel_spectrogram(y, sample_rate, n_fft, n_fft // 4, n_mels, power, normalized, False)
    return sum(mean_difference(my, mx, n) for n in ((norms,) if isinstance(norms, str) else norms))


def encodec_audio_distance(x, y, scales, sample_rate, norms, power, normalized, n_mels):
    """EncodecAudioDistance(scales, partial(SpectralDistance, ..., mel=n_mels))(x, y) as a dictionary."""
    return {"waveform_distance": mean_difference(y, x, "L1"),
            "spectral_distance": sum(spectral_distance(x, y, s, sample_rate, norms, power, normalized, n_mels) for s in scales)}


def white_noise(shape, seed, dtype=torch.float32, amplitude=1.0):
    g = torch.Generator().manual_seed(seed)
    return amplitude * torch.randn(*shape, generator=g, dtype=dtype)
