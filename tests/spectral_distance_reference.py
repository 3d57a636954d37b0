"""Test-side reference of the plain ``core.SpectralDistance`` / ``core.EncodecAudioDistance`` (rave/core.py:415-490 without
``mel``; a plain helper module, no fixtures): torchaudio ``Spectrogram(n_fft, hop_length = n_fft / 4, power, normalized,
center=False)`` of both signals -- periodic Hann window, frames of n_fft samples every hop, no padding, one-sided spectrum,
divided by sqrt(sum(window^2)) when normalised, ``|.|^power`` -- then ``mean_difference(y, x, norm)`` summed over the norms.
Everything runs in the dtype of the input: float64 inputs give the float64 reference, and autograd through it the reference
gradient.  The framing, the magnitude (sqrt(re^2 + im^2) of the two planes) and ``mean_difference`` are those of
tests/mel_distance_reference.py.
"""
import torch

from mel_distance_reference import mean_difference, smallest_relative_bin, spectrum, white_noise  # noqa: F401


def power_spectrum(x, n_fft, power, normalized):
    """(..., T) -> (..., frames, bins): |S|^power in x's dtype."""
    re, im = spectrum(x, n_fft, n_fft // 4, normalized, False)
    p = re * re + im * im
    if power == 1:
        return p.sqrt()
    assert power == 2
    return p


def spectral_distance(x, y, n_fft, norms, power, normalized):
    """SpectralDistance(n_fft, sr, norms, power, normalized)(x, y): hop n_fft / 4, center=False."""
    sx, sy = power_spectrum(x, n_fft, power, normalized), power_spectrum(y, n_fft, power, normalized)
    return sum(mean_difference(sy, sx, n) for n in ((norms,) if isinstance(norms, str) else norms))


def encodec_audio_distance(x, y, scales, norms, power, normalized):
    """EncodecAudioDistance(scales, partial(SpectralDistance, ...))(x, y) as a dictionary."""
    return {"waveform_distance": mean_difference(y, x, "L1"),
            "spectral_distance": sum(spectral_distance(x, y, s, norms, power, normalized) for s in scales)}


def smallest_gap(x, y, n_fft, normalized):
    """min |A - B| / max(A, B) over all elements at power 1, in float64: how close the L1 term comes to its kink at A = B.  A
    float32 transform is off by 1e-7 ... 3e-7 of the peak bin, so an element closer than that may take either sign in any
    float32 implementation, torch's included."""
    a, b = power_spectrum(y.double(), n_fft, 1, normalized), power_spectrum(x.double(), n_fft, 1, normalized)
    return float(((a - b).abs() / torch.maximum(a, b)).min())


def kink_clear(x, y, n_fft, normalized):
    """The two conditions under which the power-1 / L1 gradient is well conditioned in float32: no element within 1e-5 of the
    kink, no bin of either signal within 1e-6 of zero relative to its row's peak."""
    return (smallest_gap(x, y, n_fft, normalized) > 1e-5
            and smallest_relative_bin(x, n_fft, n_fft // 4, normalized, False) > 1e-6
            and smallest_relative_bin(y, n_fft, n_fft // 4, normalized, False) > 1e-6)
