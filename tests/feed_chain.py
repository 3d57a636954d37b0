"""The per-item transform chain of the reference's ``get_dataset`` (rave/dataset.py:207-261) restated with numpy / scipy for
injected draws, with the two steps behind ``rave train --normalize`` / ``--derivative``: crop (after RandomPitch =
scipy.signal.resample_poly of the whole item), the all-pass phase mangle through lfilter, Dequantize with injected noise,
normalize_signal, the derivator, RandomMute, float32.  No GPU; shared by tests/test_feed_normalize_host.py and
tests/test_gpu_feed_normalize.py, which also take their inputs (``make_pcm``, the draws below) from here.

Two dtype variants:
  ``ref32``  the dtypes the reference holds under the installed numpy: the item is float32, lfilter (and so every filtered
             item, and everything behind the derivator) is float64, Dequantize adds in place (an unfiltered item stays
             float32 through normalize_signal); the result is float32.
  ``ref64``  everything in float64, never rounded; the result is float64.
"""
import numpy as np
from scipy.signal import lfilter, resample_poly

N_ITEMS, CH, LENGTH, N = 6, 2, 6000, 4352   # n_signal = one full 4096-sample chunk of the kernel plus a ragged one
FULL, QUIET, LOUD1, ZERO = 0, 1, 2, 3       # items 4 and 5 are ordinary
MAX_GAIN_DB = 30

ITEMS = np.arange(N_ITEMS)
IN_POINTS = np.array([0, 1648, 777, 5, 1001, 333])                 # 1648 = LENGTH - N: both ends of the item
ANGLES = [0.05, None, 0.2, None, 0.003, None]                      # all-pass on for some items, off for the others
ANGLES_FLIPPED = [None, 0.7, None, 0.1, None, 0.02]
PITCH_RANGE = (0.73, 1.4)                                          # every ratio leaves at least N of the 6000 samples
RATIOS = [(13, 10), None, (14, 19), None, (18, 19), None]
PITCH_IN_POINTS = np.array([7800 - N, 1648, 4422 - N, 5, 321, 333])  # ceil(6000 up / down) - N: the zero-padded far edge


def make_pcm() -> np.ndarray:
    """(6, 2, 6000) int16: full-scale noise; an item of amplitude <= 100 (peak below -30 dB: the gain cap); an item that is
    loud in channel 1 only (the peak of the item is not in its first row); an all-zero item; two ordinary items."""
    rng = np.random.default_rng(7)
    x = np.zeros((N_ITEMS, CH, LENGTH), dtype=np.int64)
    x[FULL] = rng.integers(-32768, 32768, (CH, LENGTH))
    x[FULL, 0, 100], x[FULL, 1, 200] = -32768, 32767               # the extremes themselves, inside every crop of this item
    x[QUIET] = rng.integers(-100, 101, (CH, LENGTH))
    x[LOUD1, 0] = rng.integers(-300, 301, LENGTH)
    x[LOUD1, 1] = rng.integers(-20000, 20001, LENGTH)
    x[4] = rng.integers(-12000, 12000, (CH, LENGTH)) + np.array([5000, -7000])[:, None]
    x[5] = rng.integers(-9000, 9000, (CH, LENGTH))
    return x.astype(np.int16)


def make_noise(batch: int = N_ITEMS, seed: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).random((batch * CH, N)).astype(np.float32)


def gain_of(peak, max_gain_db=MAX_GAIN_DB):
    """The gain normalize_signal applies to an item of this peak (rave/dataset.py:196-204), in the dtype of ``peak``."""
    if peak == 0:
        return 1.0
    level_db = 20 * np.log10(peak)
    return 10 ** (min(max_gain_db, -level_db) / 20)


def normalize_signal(x: np.ndarray, max_gain_db=MAX_GAIN_DB) -> np.ndarray:
    peak = np.max(abs(x))
    return x if peak == 0 else x * gain_of(peak, max_gain_db)


def derivator(x: np.ndarray) -> np.ndarray:
    """y[n] = 0.5 x[n] - 0.5 x[n - 1], zero initial state (rave/dataset.py:24-29); float64 whatever the input."""
    return lfilter([.5, -.5], [1], x)


def allpass(angle: float, x: np.ndarray) -> np.ndarray:
    z0 = .99 * np.exp(1j * angle)                                  # rave/dataset.py:290-299, amplitude .99
    aa = [1.0, -2.0 * float(np.real(z0)), float(abs(z0) ** 2)]
    bb = [float(abs(z0) ** 2), -2.0 * float(np.real(z0)), 1.0]
    return lfilter(bb, aa, x)


def dequantized(pcm, noise, items, in_points, angles, ratios=None, variant="ref64", n=N):
    """The items up to and including Dequantize(16): a list of (CH, n) arrays in the dtype the variant holds there."""
    assert variant in ("ref32", "ref64")
    out = []
    for b in range(len(items)):
        x = pcm[items[b]].astype(np.float32) / (2 ** 15 - 1)
        if variant == "ref64":
            x = x.astype(np.float64)
        if ratios is not None and ratios[b] is not None:
            x = resample_poly(x, ratios[b][0], ratios[b][1], padtype="mean", axis=-1)
        x = x[..., in_points[b]:in_points[b] + n].copy()
        assert x.shape == (CH, n)
        if angles[b] is not None:
            x = allpass(angles[b], x)
        x += noise[CH * b:CH * b + CH].astype(np.float64) / 2 ** 16          # in place, as transforms.Dequantize
        out.append(x)
    return out


def chain(pcm, noise, items, in_points, angles, ratios=None, mute=None, normalize=False, derivative=False,
          max_gain_db=MAX_GAIN_DB, variant="ref64", n=N) -> np.ndarray:
    """(batch, CH, n): float32 for ``ref32`` (the chain's last astype), float64 for ``ref64`` (never rounded)."""
    rows = dequantized(pcm, noise, items, in_points, angles, ratios, variant, n)
    out = np.empty((len(rows), CH, n), dtype=np.float32 if variant == "ref32" else np.float64)
    for b, x in enumerate(rows):
        if normalize:
            x = normalize_signal(x, max_gain_db)
        if derivative:
            x = derivator(x)
        if mute is not None and mute[b]:
            x = x * 0
        out[b] = x
    return out


def row_bound(ref32: np.ndarray, ref64: np.ndarray) -> float:
    """The bar of one row: max |got - ref64| <= 2 max |ref32 - ref64| + 2^-23 max |ref64| (tests/test_gpu_feed_pitch.py)."""
    return 2 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 2.0 ** -23 * float(np.abs(ref64).max())
