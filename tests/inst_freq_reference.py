"""Torch restatement of WeightedInstantaneousSpectralDistance over MultiScaleSTFT(magnitude=False) (rave/core.py:269-319,
:347-412) in a chosen dtype, cumsum included -- the yardstick of tests/test_inst_freq_host.py and tests/test_gpu_inst_freq.py.
It depends on torch alone."""
import math

import torch


def stft(x, n_fft, normalized):
    """(rows, T) -> complex (rows, bins, frames): Spectrogram(n_fft, hop = n_fft / 4, center, reflect, normalized, power=None)."""
    w = torch.hann_window(n_fft, dtype=x.dtype, device=x.device)
    s = torch.stft(x, n_fft, hop_length=n_fft // 4, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    if normalized:
        s = s / w.pow(2.).sum().sqrt()
    return s


def derivative(x):
    return x[..., 1:] - x[..., :-1]


def unwrap(x):
    x = derivative(x)
    x = (x + math.pi) % (2 * math.pi)
    return (x - math.pi).cumsum(-1)


def inst_freq(phase):
    """rave/core.py:356-368, literally: derivative(unwrap(phase)) along the frames."""
    return derivative(unwrap(phase))


def distance(target, pred, scales, normalized, weighted, dtype=torch.float64):
    """-> (spectral_distance, phase_distance, [(IFx, IFy) per scale, unweighted, (rows, bins, frames - 2)]) in ``dtype``; the
    scalars are differentiable in ``target`` and ``pred`` when those require grad (pass tensors of ``dtype`` then)."""
    target, pred = target.to(dtype), pred.to(dtype)
    target, pred = target.reshape(-1, target.shape[-1]), pred.reshape(-1, pred.shape[-1])
    spectral, phase, ifs = 0., 0., []
    for n in scales:
        x, y = stft(target, int(n), normalized), stft(pred, int(n), normalized)
        xa, ya = x.abs(), y.abs()
        d = xa - ya
        spectral = spectral + (d * d).mean() / (xa * xa).mean() + (torch.log1p(xa) - torch.log1p(ya)).abs().mean()
        fx, fy = inst_freq(x.angle()), inst_freq(y.angle())
        ifs.append((fx.detach(), fy.detach()))
        if weighted:
            mask = torch.clip(torch.log1p(xa[..., 2:]), 0, 1)
            fx, fy = fx * mask, fy * mask
        e = fx - fy
        phase = phase + (e * e).mean()
    return spectral, phase, ifs
