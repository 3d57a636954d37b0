"""FrequencyMasking (rave/transforms.py:180-195) two ways, in float64, for the tests of rh_feed_freq_mask_f32 and of
``GpuBatchFeed(freq_mask=...)``: ``reference`` is the reference's own expression, scipy.signal.istft of the masked
scipy.signal.stft; ``model`` is the formulation the kernel is built on (rave_amd/csrc/feed_mask.hip) -- x minus the band
component, hop block by hop block, from the two frames that cover the block.  No GPU; shared by tests/test_feed_mask_host.py
and tests/test_gpu_feed_mask.py, which also take their inputs from here."""
import numpy as np
import scipy.signal

NPERSEG, HOP, BINS = 4096, 2048, 2049
LENGTHS = (4096, 6144, 8192)                       # 3, 4 and 5 frames: first and last block, odd and even hop count
BANDS = ((0, 1), (2047, 1), (0, 79), (1969, 79), (1000, 40))     # (freq_idx, mask_size): both ends, one bin and the widest default
BAR = 1e-4                                         # the project's parity bar: relative L2 per row


def make_rows(n_rows: int, n: int, seed: int = 3) -> np.ndarray:
    """Unit-variance noise, float32 values held in float64 (the kernel's input is float32)."""
    return np.random.default_rng(seed + n).standard_normal((n_rows, n)).astype(np.float32).astype(np.float64)


def reference(x: np.ndarray, band) -> np.ndarray:
    """rave/transforms.py:186-195 for one drawn band, without the final astype; ``band`` None = the item itself."""
    if band is None:
        return x
    freq_idx, mask_size = band
    spectrogram = scipy.signal.stft(x, nperseg=NPERSEG)[2]
    assert spectrogram.shape[-2] == BINS
    spectrogram[..., freq_idx:freq_idx + mask_size, :] = 0
    return scipy.signal.istft(spectrogram, nperseg=NPERSEG)[1]


def model(x: np.ndarray, band) -> np.ndarray:
    """y[2048 b + j] = x[2048 b + j] - (w[j] h_{b+1}[j] + w[j + 2048] h_b[j + 2048]) / (w[j]^2 + w[j + 2048]^2) with
    h_t = irfft(B . rfft(w . xpad_t)), xpad_t = the samples [2048 (t - 1), 2048 (t + 1)) of x, zero outside the row."""
    if band is None:
        return x
    freq_idx, mask_size = band
    n = x.shape[-1]
    assert n % HOP == 0 and n >= NPERSEG
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(NPERSEG) / NPERSEG)
    keep = np.zeros(BINS)
    keep[freq_idx:freq_idx + mask_size] = 1
    xpad = np.concatenate([np.zeros(x.shape[:-1] + (HOP,)), x, np.zeros(x.shape[:-1] + (HOP,))], -1)
    h = [np.fft.irfft(keep * np.fft.rfft(w * xpad[..., t * HOP:t * HOP + NPERSEG]), NPERSEG) for t in range(n // HOP + 1)]
    y = np.empty_like(x)
    for b in range(n // HOP):
        num = w[:HOP] * h[b + 1][..., :HOP] + w[HOP:] * h[b][..., HOP:]
        y[..., b * HOP:(b + 1) * HOP] = x[..., b * HOP:(b + 1) * HOP] - num / (w[:HOP] ** 2 + w[HOP:] ** 2)
    return y


def rel_l2(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))
