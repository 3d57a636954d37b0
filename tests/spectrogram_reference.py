"""torchaudio.transforms.Spectrogram's documented steps restated in plain torch, for float64: pad (reflect, when centred),
frame, window, one-sided ``rfft``, normalise by sqrt(sum(window^2)), then ``power``.  Differentiable, so float64 autograd
through it is the reference gradient.  tests/test_spectrogram_host.py checks it against ``torch.stft`` in float64 and, where
one is installed, against torchaudio itself."""
import torch
import torch.nn.functional as F


def frames_of(n_fft, hop, t, center):
    return t // hop + 1 if center else (t - n_fft) // hop + 1


def spectrogram(x, window, n_fft, hop, normalized, center, power=None):
    """x (..., T) -> (..., n_fft // 2 + 1, frames): complex for ``power=None``, else |s| ** power, in x's dtype."""
    window = window.to(x.dtype)
    shape = x.shape
    x = x.reshape(-1, shape[-1])
    if center:
        x = F.pad(x.unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect").squeeze(1)
    fr = x.unfold(-1, n_fft, hop)                               # (rows, frames, n_fft)
    s = torch.fft.rfft(fr * window, dim=-1).transpose(-1, -2)   # (rows, bins, frames)
    if normalized:
        s = s / window.pow(2).sum().sqrt()
    s = s.reshape(shape[:-1] + s.shape[-2:])
    if power is None:
        return s
    return s.abs() if power == 1 else s.real.pow(2) + s.imag.pow(2)


def real_imag(x, window, n_fft, hop, normalized, center):
    """x (B, C, T) -> the reference's ``cat([s.real, s.imag], 1)`` (B, 2 C, bins, frames) (rave/discriminator.py:147-152)."""
    s = spectrogram(x, window, n_fft, hop, normalized, center)
    return torch.cat([s.real, s.imag], 1)


def planes(x, window, n_fft, hop, normalized, center):
    """x (..., T) -> (..., 2, bins, frames): real part, imaginary part."""
    s = spectrogram(x, window, n_fft, hop, normalized, center)
    return torch.stack([s.real, s.imag], -3)


def white_noise(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
