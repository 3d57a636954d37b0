"""Stand-in for ``torchaudio.transforms.MelSpectrogram`` as configs/hybrid.gin binds it (``RAVE.spectrogram``, the encoder
input of ``RAVE.input_mode = "mel"``, rave/model.py:238-242): torchaudio's constructor, and its two buffers under torchaudio's
names -- ``spectrogram.window`` (n_fft,) and ``mel_scale.fb`` (n_fft // 2 + 1, n_mels) -- so that a reference checkpoint
loads.  GPU tensors run ONE HIP kernel (rave_amd/csrc/mel.hip: framing, window, FFT, power, mel sums; ``log_mel`` also the
reference's log1p and dropped last frame); CPU tensors run the torch composition.  What the kernel does not implement raises
at construction.  No backward: nothing trainable is upstream of the audio, the result never requires grad.

``DifferentiableMelSpectrogram`` (below) is the class the mel variant of ``losses.SpectralDistance`` holds: the same transform
WITH the gradient with respect to the audio, power 1 or 2, frames centred or not.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """``torchaudio.functional.melscale_fbanks(..., norm=None, mel_scale="htk")``: (n_freqs, n_mels) triangular filters,
    fb[f, m] = max(0, min(down, up)), in float32 as torchaudio computes them."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


class _Window(nn.Module):
    """Holder of ``spectrogram.window`` (torchaudio.transforms.Spectrogram's buffer)."""

    def __init__(self, n_fft: int):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft))


class _FilterBank(nn.Module):
    """Holder of ``mel_scale.fb`` (torchaudio.transforms.MelScale's buffer)."""

    def __init__(self, fb: torch.Tensor):
        super().__init__()
        self.register_buffer("fb", fb)


class MelSpectrogram(nn.Module):
    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, win_length: Optional[int] = None,
                 hop_length: Optional[int] = None, f_min: float = 0.0, f_max: Optional[float] = None, pad: int = 0,
                 n_mels: int = 128, window_fn=torch.hann_window, power: float = 2.0, normalized: bool = False,
                 wkwargs: Optional[dict] = None, center: bool = True, pad_mode: str = "reflect", onesided: Optional[bool] = None,
                 norm: Optional[str] = None, mel_scale: str = "htk"):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        for what, bad in (("power != 2", power != 2), ("center=False", not center), (f"pad_mode={pad_mode!r}", pad_mode != "reflect"),
                          (f"mel_scale={mel_scale!r}", mel_scale != "htk"), (f"norm={norm!r}", norm is not None),
                          ("win_length != n_fft", win_length != n_fft), ("pad != 0", pad != 0),
                          ("a window_fn other than torch.hann_window", window_fn is not torch.hann_window or bool(wkwargs)),
                          ("onesided=False", onesided is not None and not onesided)):
            if bad:
                raise NotImplementedError(f"rave_amd.MelSpectrogram: {what} is not built (rave_amd/csrc/mel.hip)")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length = int(sample_rate), int(n_fft), int(win_length), int(hop_length)
        self.n_mels, self.normalized = int(n_mels), bool(normalized)
        self.f_min = float(f_min)
        self.f_max = float(f_max) if f_max is not None else float(self.sample_rate // 2)
        self.spectrogram = _Window(self.n_fft)
        self.mel_scale = _FilterBank(melscale_fbanks(self.n_fft // 2 + 1, self.f_min, self.f_max, self.n_mels, self.sample_rate))
        self._tables = {}

    # ---- the torch composition (CPU tensors; also what tools/bench_mel.py times on the GPU: what torchaudio would launch)
    def compose(self, x: torch.Tensor) -> torch.Tensor:
        """(..., T) -> (..., n_mels, T // hop + 1): torch.stft, |.|^2, the filterbank product."""
        win, fb = self.spectrogram.window.to(x.dtype), self.mel_scale.fb.to(x.dtype)
        shape = x.shape
        s = torch.stft(x.reshape(-1, shape[-1]), self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=win,
                       center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        if self.normalized:
            s = s / win.pow(2.0).sum().sqrt()
        mel = torch.matmul(s.abs().pow(2.0).transpose(-1, -2), fb).transpose(-1, -2)
        return mel.reshape(shape[:-1] + mel.shape[-2:])

    def _device_tables(self, dev):
        """(bins, scale) for the kernel: per filter the range [lo, hi) of its non-zero bins, read from the CURRENT ``fb`` buffer
        (a loaded checkpoint's), and 1 / sum(window^2); cached per device and buffer version, made outside any capture."""
        win, fb = self.spectrogram.window, self.mel_scale.fb
        key = (str(dev), fb.data_ptr(), fb._version, win.data_ptr(), win._version)
        hit = self._tables.get("key") == key
        if not hit:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("rave_amd.MelSpectrogram: first call inside a hipGraph capture (run one eager step first)")
            nz = fb.detach().cpu() != 0
            idx = torch.arange(fb.shape[0]).unsqueeze(1)
            lo = torch.where(nz, idx, fb.shape[0]).min(0).values
            hi = torch.where(nz, idx + 1, 0).max(0).values
            lo = torch.minimum(lo, hi)                      # an all-zero filter: the empty range [0, 0)
            bins = torch.stack([lo, hi], 1).to(torch.int32).contiguous().to(dev)
            scale = 1.0 / float(win.detach().double().pow(2).sum()) if self.normalized else 1.0
            self._tables = {"key": key, "bins": bins, "scale": scale}
        return self._tables["bins"], self._tables["scale"]

    def refresh_host_caches(self) -> None:
        """GraphedTrainingStep calls this before it records (its state restore rewrote the buffers, which bumps their version
        counters): the tables are rebuilt here, outside the capture."""
        if self.mel_scale.fb.is_cuda:
            self._device_tables(self.mel_scale.fb.device)

    def _run(self, x: torch.Tensor, log1p: bool, drop_last: bool) -> torch.Tensor:
        if not x.is_cuda:
            with torch.no_grad():
                y = self.compose(x)
                if drop_last:
                    y = y[..., :-1]
                return torch.log1p(y) if log1p else y
        from . import ops
        bins, scale = self._device_tables(x.device)
        return ops.mel_spectrogram(x, self.spectrogram.window, self.mel_scale.fb, bins, self.hop_length, scale, log1p, drop_last)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """torchaudio's result: (..., T) -> (..., n_mels, T // hop + 1), power mel spectrogram."""
        return self._run(x, False, False)

    def log_mel(self, x: torch.Tensor) -> torch.Tensor:
        """``log1p(self(x)[..., :-1])`` (rave/model.py:240-241) in the same launch: (..., T) -> (..., n_mels, T // hop)."""
        return self._run(x, True, True)


def filter_bins(fb: torch.Tensor) -> torch.Tensor:
    """(n_mels, 2) int32 on the host: per filter the range [lo, hi) of its non-zero bins in ``fb`` (n_freqs, n_mels); an
    all-zero filter gets the empty range [0, 0)."""
    nz = fb.detach().cpu() != 0
    idx = torch.arange(fb.shape[0]).unsqueeze(1)
    lo = torch.where(nz, idx, fb.shape[0]).min(0).values
    hi = torch.where(nz, idx + 1, 0).max(0).values
    return torch.stack([torch.minimum(lo, hi), hi], 1).to(torch.int32).contiguous()


class DifferentiableMelSpectrogram(nn.Module):
    """``torchaudio.transforms.MelSpectrogram`` WITH its gradient with respect to the audio: the spectrum of
    ``core.SpectralDistance(mel=n)`` (rave/core.py:458-468), where both signals of the loss pass through it.  torchaudio's
    constructor and buffers (``spectrogram.window``, ``mel_scale.fb``); ``power`` 1 or 2, ``center`` True or False.  GPU float32
    tensors of a built size run rave_amd/csrc/mel.hip (rh_mel_diff_fwd_f32 / rh_mel_diff_bwd_f32: one launch per direction);
    everything else takes the torch composition (rave_amd.ops.mel_spectrogram_diff).  Beside ``MelSpectrogram`` (the encoder
    input: forward only, centred, power 2), which it does not replace."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, win_length: Optional[int] = None,
                 hop_length: Optional[int] = None, f_min: float = 0.0, f_max: Optional[float] = None, pad: int = 0,
                 n_mels: int = 128, window_fn=torch.hann_window, power: float = 2.0, normalized: bool = False,
                 wkwargs: Optional[dict] = None, center: bool = True, pad_mode: Optional[str] = "reflect",
                 onesided: Optional[bool] = None, norm: Optional[str] = None, mel_scale: str = "htk"):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        # (pad_mode is read only for centred frames, as by torch.stft: rave/core.py passes center=False, pad_mode=None)
        for what, bad in (("power=None", power is None), (f"power={power!r} (1 and 2 are built)", power is not None and power not in (1, 2)),
                          (f"pad_mode={pad_mode!r}", bool(center) and pad_mode != "reflect"),
                          (f"mel_scale={mel_scale!r}", mel_scale != "htk"), (f"norm={norm!r}", norm is not None),
                          ("win_length != n_fft", win_length != n_fft), ("pad != 0", pad != 0),
                          ("a window_fn other than torch.hann_window", window_fn is not torch.hann_window or bool(wkwargs)),
                          ("onesided=False", onesided is not None and not onesided)):
            if bad:
                raise NotImplementedError(f"rave_amd.DifferentiableMelSpectrogram: {what} is not built (rave_amd/csrc/mel.hip)")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length = int(sample_rate), int(n_fft), int(win_length), int(hop_length)
        self.n_mels, self.normalized, self.power, self.center = int(n_mels), bool(normalized), int(power), bool(center)
        self.f_min = float(f_min)
        self.f_max = float(f_max) if f_max is not None else float(self.sample_rate // 2)
        self.spectrogram = _Window(self.n_fft)
        self.mel_scale = _FilterBank(melscale_fbanks(self.n_fft // 2 + 1, self.f_min, self.f_max, self.n_mels, self.sample_rate))
        self._tables = {}

    def _host_scale(self) -> float:
        """1 / sqrt(sum(window^2)) of ``normalized=True`` from the CURRENT window, in float64; 1.0 otherwise."""
        return float(self.spectrogram.window.detach().double().pow(2).sum().rsqrt()) if self.normalized else 1.0

    def _device_tables(self, dev):
        """(bins, scale) for the kernels, read from the CURRENT buffers (a loaded checkpoint's); cached per device and buffer
        version, made outside any capture."""
        win, fb = self.spectrogram.window, self.mel_scale.fb
        key = (str(dev), fb.data_ptr(), fb._version, win.data_ptr(), win._version)
        if self._tables.get("key") != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("rave_amd.DifferentiableMelSpectrogram: first call inside a hipGraph capture (run one eager step first)")
            self._tables = {"key": key, "bins": filter_bins(fb).to(dev), "scale": self._host_scale()}
        return self._tables["bins"], self._tables["scale"]

    def refresh_host_caches(self) -> None:
        """GraphedTrainingStep calls this before it records (its state restore rewrote the buffers, which bumps their version
        counters): the tables are rebuilt here, outside the capture."""
        if self.mel_scale.fb.is_cuda:
            self._device_tables(self.mel_scale.fb.device)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(..., T) -> (..., n_mels, frames), frames = T // hop + 1 centred and (T - n_fft) // hop + 1 uncentred."""
        from . import ops
        if x.is_cuda:
            bins, scale = self._device_tables(x.device)
        else:
            bins, scale = None, self._host_scale()
        return ops.mel_spectrogram_diff(x, self.spectrogram.window, self.mel_scale.fb, bins, self.n_fft, self.hop_length, scale,
                                        self.power, self.center)
