"""Test-side reference of ``torchaudio.transforms.MelSpectrogram`` (a plain helper module, no fixtures): torchaudio is not
installed where the tests run, so the reference of the mel encoder input (rave/model.py:238-242) is this torch composition of
torchaudio's documented steps -- periodic Hann window, ``center=True`` with reflect padding of n_fft / 2, one-sided spectrum,
divided by sqrt(sum(window^2)) when ``normalized``, |.|^2, ``MelScale(f_min=0, f_max=sample_rate // 2, mel_scale="htk",
norm=None)`` -- with torchaudio's constructor arguments and buffer names (``spectrogram.window``, ``mel_scale.fb``).
``.double()`` gives the float64 reference the GPU tests compare with.  Written apart from rave_amd/mel.py on purpose: the
framing here is an explicit pad + unfold + rfft, not torch.stft.
"""
import math

import torch
import torch.nn as nn


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, dtype=torch.float32):
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk"): fb[f, m] = max(0, min(down, up)), (n_freqs, n_mels)."""
    freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_lo = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_hi = 2595.0 * math.log10(1.0 + f_max / 700.0)
    mels = torch.linspace(m_lo, m_hi, n_mels + 2, dtype=dtype)
    edges = 700.0 * (10.0 ** (mels / 2595.0) - 1.0)              # n_mels + 2 band edges in Hz
    width = edges[1:] - edges[:-1]
    dist = edges[None, :] - freqs[:, None]                      # (n_freqs, n_mels + 2)
    down = -dist[:, :-2] / width[:-1]
    up = dist[:, 2:] / width[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


class _Spectrogram(nn.Module):
    def __init__(self, n_fft):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft, periodic=True))


class _MelScale(nn.Module):
    def __init__(self, fb):
        super().__init__()
        self.register_buffer("fb", fb)


class MelSpectrogram(nn.Module):
    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0, n_mels=128,
                 window_fn=torch.hann_window, power=2.0, normalized=False, wkwargs=None, center=True, pad_mode="reflect",
                 onesided=None, norm=None, mel_scale="htk"):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        assert (power, center, pad_mode, norm, mel_scale, pad, win_length) == (2.0, True, "reflect", None, "htk", 0, n_fft)
        assert window_fn is torch.hann_window and not wkwargs and onesided in (None, True)
        self.n_fft, self.hop_length, self.normalized = n_fft, (win_length // 2 if hop_length is None else hop_length), normalized
        self.spectrogram = _Spectrogram(n_fft)
        f_max = float(sample_rate // 2) if f_max is None else f_max
        self.mel_scale = _MelScale(melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate))

    def forward(self, x):
        """(..., T) -> (..., n_mels, T // hop + 1) in x's dtype (the buffers are cast to it)."""
        w, fb = self.spectrogram.window.to(x.dtype), self.mel_scale.fb.to(x.dtype)
        lead, t = x.shape[:-1], x.shape[-1]
        half = self.n_fft // 2
        xp = torch.nn.functional.pad(x.reshape(-1, 1, t), (half, half), mode="reflect")[:, 0]
        frames = xp.unfold(-1, self.n_fft, self.hop_length) * w                      # (rows, frames, n_fft)
        spec = torch.fft.rfft(frames, dim=-1)
        if self.normalized:
            spec = spec / w.pow(2).sum().sqrt()
        power = spec.real ** 2 + spec.imag ** 2                                     # (rows, frames, bins)
        mel = (power @ fb).transpose(-1, -2)                                        # (rows, n_mels, frames)
        return mel.reshape(*lead, *mel.shape[-2:])


def log_mel(module, x):
    """rave/model.py:238-242 (`RAVE._mel_encode`): (*batch, C, T) -> (*batch, C * n_mels, T // hop)."""
    batch = x.shape[:-2]
    m = module(x)[..., :-1]
    return torch.log1p(m).reshape(*batch, -1, m.shape[-1])


def white_noise(shape, amplitude, seed):
    """Seeded white noise whose rows and channels all differ."""
    g = torch.Generator().manual_seed(seed)
    return amplitude * torch.randn(*shape, generator=g)


def onset(seed=5, n=8192, quiet=1e-4):
    """(1, 1, n): white noise at `quiet` for the first half, then at amplitude 1."""
    x = white_noise((1, 1, n), 1.0, seed)
    x[..., : n // 2] *= quiet
    return x


def tones(n_fft, t, bins):
    """(len(bins), 1, t): row i is a sine at the centre of bin bins[i]."""
    n = torch.arange(t, dtype=torch.float64)
    return torch.stack([torch.sin(2 * math.pi * b * n / n_fft) for b in bins]).unsqueeze(1).float()
