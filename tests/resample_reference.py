"""``transforms.Resample`` of the reference (rave/transforms.py:31-40) restated without torchaudio, which is not installed:
``torchaudio.functional.resample(torch.from_numpy(x).float(), orig, new).numpy()`` with torchaudio's defaults is, in torchaudio
0.12 - 2.x, ``_get_sinc_resample_kernel`` (sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99) followed by
``_apply_sinc_resample_kernel`` -- a zero-padded, strided ``conv1d`` whose ``new / gcd`` filter outputs are interleaved and cut to
``ceil(new * length / orig)`` samples.  Both are written out below with torch CPU ops, and combined with tests/feed_chain.py
into the chain ``get_dataset`` builds for a dataset stored at another rate (rave/dataset.py:238-250): Dequantize -> Resample ->
normalize_signal -> derivator -> RandomMute -> float32.  No GPU; shared by tests/test_feed_resample_host.py and
tests/test_gpu_feed_resample.py.

Two dtype variants, as in tests/feed_chain.py:
  ``ref32``  the reference's dtypes: the item behind Dequantize goes through ``.float()``, the taps are built in float32, the
             convolution runs in float32, normalize_signal stays in float32, everything behind the derivator is float64; the
             result is float32.
  ``ref64``  everything in float64 (the taps included), never rounded; the result is float64.
"""
import math

import numpy as np
import torch

import feed_chain as F

# (orig, new) -> o / n, (width, K), n_res at n_signal = 4352; computed from the formula, not from the code under test
RATIOS = {(48000, 44100): ((160, 147), (7, 174), 3999), (44100, 48000): ((147, 160), (7, 161), 4737),
          (88200, 44100): ((2, 1), (13, 28), 2176), (22050, 44100): ((1, 2), (7, 15), 8704),
          (44100, 32000): ((441, 320), (9, 459), 3158)}
ENVELOPE = (16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def reduced(orig: int, new: int):
    g = math.gcd(orig, new)
    return orig // g, new // g


def sinc_kernel(orig: int, new: int, dtype=torch.float32):
    """_get_sinc_resample_kernel for a waveform of ``dtype``: the (n, K) table and ``width``."""
    o, n = reduced(orig, new)
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    idx = torch.arange(-width, width + o, dtype=dtype)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=dtype)[:, None, None] / n + idx
    t *= base
    t.clamp_(-6, 6)
    window = torch.cos(t * math.pi / 6 / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t) * (window * (base / o))
    assert kernels.shape == (n, 1, 2 * width + o) and kernels.dtype == dtype
    return kernels[:, 0], width


def resampled_length(length: int, orig: int, new: int) -> int:
    o, n = reduced(orig, new)
    return int(math.ceil(n * length / o))


def apply_kernel(x: torch.Tensor, table: torch.Tensor, width: int, orig: int, new: int) -> torch.Tensor:
    """_apply_sinc_resample_kernel on rows (..., L) in the dtype of ``x`` and ``table``."""
    o, n = reduced(orig, new)
    shape, length = x.shape, x.shape[-1]
    x = torch.nn.functional.pad(x.reshape(-1, length), (width, width + o))
    y = torch.nn.functional.conv1d(x[:, None], table[:, None], stride=o)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)
    return y[..., :resampled_length(length, orig, new)].reshape(shape[:-1] + (-1,))


def resample(x: np.ndarray, orig: int, new: int, variant: str) -> np.ndarray:
    """Resample.__call__ on one item (CH, L): float32 in ``ref32`` whatever the dtype of ``x``, float64 in ``ref64``."""
    if orig == new:
        return x
    dtype = torch.float32 if variant == "ref32" else torch.float64
    table, width = sinc_kernel(orig, new, dtype)
    return apply_kernel(torch.from_numpy(np.ascontiguousarray(x)).to(dtype), table, width, orig, new).numpy()


def kernel_arithmetic(x: np.ndarray, orig: int, new: int) -> np.ndarray:
    """What the HIP kernel is specified to compute: float32 taps times the float32-rounded input, summed in float64, rounded
    once to float32.  (conv1d in float64 sums in its own order; the products are exact, so the two differ by float64 rounding
    only.)"""
    table, width = sinc_kernel(orig, new, torch.float32)
    x32 = torch.from_numpy(np.ascontiguousarray(x)).float()
    return apply_kernel(x32.double(), table.double(), width, orig, new).float().numpy()


def chain(pcm, noise, items, in_points, angles, orig, new, ratios=None, mute=None, normalize=False, derivative=False,
          max_gain_db=F.MAX_GAIN_DB, variant="ref64", n=F.N) -> np.ndarray:
    """(batch, CH, n_res): tests/feed_chain.py's ``chain`` with Resample(orig, new) right behind Dequantize."""
    rows = F.dequantized(pcm, noise, items, in_points, angles, ratios, variant, n)
    out = np.empty((len(rows), F.CH, resampled_length(n, orig, new)), dtype=np.float32 if variant == "ref32" else np.float64)
    for b, x in enumerate(rows):
        x = resample(x, orig, new, variant)
        if normalize:
            x = F.normalize_signal(x, max_gain_db)
        if derivative:
            x = F.derivator(x)
        if mute is not None and mute[b]:
            x = x * 0
        out[b] = x
    return out
