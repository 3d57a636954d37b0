"""Stand-in for ``torchaudio.transforms.Spectrogram``: torchaudio's constructor and its single buffer ``window`` (n_fft,), so
that checkpoints interchange.  The reference builds the front end of both spectral discriminators from it
(rave/discriminator.py:12-20: ``power=None, normalized=True, center=False``; rave/descript_discriminator.py:153-160: centred).
GPU float32 tensors of a built size run ONE HIP kernel per direction (rave_amd/csrc/spectrogram.hip: framing, window,
transform, normalisation and the (real, imag) planes in the discriminators' layout; backward = the exact adjoint); CPU tensors
and every other size run the torch composition.  What neither implements raises at construction, naming the argument.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn


class Spectrogram(nn.Module):
    def __init__(self, n_fft: int = 400, win_length: Optional[int] = None, hop_length: Optional[int] = None, pad: int = 0,
                 window_fn: Callable[..., torch.Tensor] = torch.hann_window, power: Optional[float] = 2.0,
                 normalized: bool = False, wkwargs: Optional[dict] = None, center: bool = True, pad_mode: str = "reflect",
                 onesided: bool = True):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        for what, bad in (("pad != 0", pad != 0), ("onesided=False", not onesided), ("win_length != n_fft", win_length != n_fft),
                          (f"pad_mode={pad_mode!r}", bool(center) and pad_mode != "reflect"),
                          (f"power={power!r}", power is not None and power not in (1, 2)),
                          (f"normalized={normalized!r}", not isinstance(normalized, bool))):
            if bad:
                raise NotImplementedError(f"rave_amd.Spectrogram: {what} is not built (rave_amd/csrc/spectrogram.hip)")
        self.n_fft, self.win_length, self.hop_length = int(n_fft), int(win_length), int(hop_length)
        self.pad, self.power, self.normalized, self.center, self.pad_mode, self.onesided = 0, power, normalized, bool(center), pad_mode, True
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        self._scale = None

    def _host_scale(self) -> Optional[float]:
        """1 / sqrt(sum(window^2)) for the kernel, from the CURRENT buffer (a loaded or overwritten window counts), cached per
        buffer version and made outside any capture."""
        if not self.normalized:
            return None
        win = self.window
        key = (str(win.device), win.data_ptr(), win._version)
        if self._scale is None or self._scale[0] != key:
            from . import ops
            self._scale = (key, ops.spectrogram_scale(win))
        return self._scale[1]

    def refresh_host_caches(self) -> None:
        """GraphedTrainingStep calls this before it records (its state restore rewrote the buffer, which bumps its version
        counter): the norm is read here, outside the capture."""
        if self.window.is_cuda:
            self._host_scale()

    def _planes(self, x: torch.Tensor, cat_channels: bool) -> torch.Tensor:
        from . import ops
        scale = self._host_scale() if x.is_cuda else None
        return ops.spectrogram(x, self.window, self.n_fft, self.hop_length, self.normalized, self.center, cat_channels=cat_channels,
                               scale=scale)

    def real_imag(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, C, T) -> ``cat([s.real, s.imag], 1)`` (B, 2 C, bins, frames) of the complex spectrogram s, as the kernel wrote it:
        no copy (rave/discriminator.py:147-152)."""
        return self._planes(x, True)

    def planes(self, x: torch.Tensor) -> torch.Tensor:
        """x (..., T) -> (..., 2, bins, frames): real part, imaginary part."""
        return self._planes(x, False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """torchaudio's result: (..., T) -> (..., n_fft // 2 + 1, frames); complex for ``power=None``, else |s| ** power."""
        p = self.planes(x)
        if self.power is None:
            return torch.view_as_complex(p.movedim(-3, -1).contiguous())
        sq = p.select(-3, 0).square() + p.select(-3, 1).square()
        return sq if self.power == 2 else sq.sqrt()
