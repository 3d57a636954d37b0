"""Losses of RAVE.training_step (rave/core.py) -- beside the HIP hot path ("next" #1).

On the GPU one STFT scale is: HIP framing kernel (centre + reflect pad + Hann) -> rocFFT R2C called through
hipFFT directly (rave_amd/fft.py) -> ONE fused HIP kernel for magnitude, linear + log distance and the three
reductions; backward: fused gradient kernel emitting the operand of the C2R adjoint of rfft -> rocFFT C2R ->
HIP framing adjoint (rave_amd.ops.stft_distance).  Only the FFT itself is library code.
There is no CPU branch: the reference's torch formulation lives in oracle/rave_oracle.py (audio_distance_v1) and is what the
parity tests compare with.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn


def mean_difference(target, value, norm: str = "L1", relative: bool = False):
    """rave/core.py:236-252."""
    diff = target - value
    if norm == "L1":
        diff = diff.abs().mean()
        if relative:
            diff = diff / target.abs().mean()
        return diff
    if norm == "L2":
        diff = (diff * diff).mean()
        if relative:
            diff = diff / (target * target).mean()
        return diff
    raise Exception(f"Norm must be either L1 or L2, got {norm}")


def _gan_kernel(score_real, score_fake) -> bool:
    """The three objectives below take the HIP kernel (rave_amd/csrc/gan_loss.hip, one head per call: two launches forward, one
    backward) on float32 scores of equal shape on one GPU; CPU tensors, other dtypes, unequal (broadcasting) shapes and
    ``RH_GAN_LOSS=0`` run the reference's torch composition."""
    if not (torch.is_tensor(score_real) and torch.is_tensor(score_fake) and score_real.is_cuda and score_fake.is_cuda
            and score_real.dtype == torch.float32 and score_fake.dtype == torch.float32
            and score_real.device == score_fake.device
            and score_real.shape == score_fake.shape and score_real.numel() > 0):
        return False
    from . import ops
    return ops.gan_loss_on()


def _gan_kernel_call(score_real, score_fake, mode: int):
    from . import ops
    return ops.gan_losses([(score_real, score_fake)], mode)[:2]


def hinge_gan(score_real, score_fake):
    """rave/core.py:151-155."""
    if _gan_kernel(score_real, score_fake):
        return _gan_kernel_call(score_real, score_fake, hinge_gan.gan_mode)
    loss_dis = (torch.relu(1 - score_real) + torch.relu(1 + score_fake)).mean()
    return loss_dis, -score_fake.mean()


def ls_gan(score_real, score_fake):
    """rave/core.py:158-162."""
    if _gan_kernel(score_real, score_fake):
        return _gan_kernel_call(score_real, score_fake, ls_gan.gan_mode)
    loss_dis = ((score_real - 1).pow(2) + score_fake.pow(2)).mean()
    return loss_dis, (score_fake - 1).pow(2).mean()


def nonsaturating_gan(score_real, score_fake):
    """rave/core.py:165-170: sigmoid, then clamp, then log -- the saturation at -log 1e-7 is part of the objective."""
    if _gan_kernel(score_real, score_fake):
        return _gan_kernel_call(score_real, score_fake, nonsaturating_gan.gan_mode)
    score_real = torch.clamp(torch.sigmoid(score_real), 1e-7, 1 - 1e-7)
    score_fake = torch.clamp(torch.sigmoid(score_fake), 1e-7, 1 - 1e-7)
    loss_dis = -(torch.log(score_real) + torch.log(1 - score_fake)).mean()
    return loss_dis, -torch.log(score_fake).mean()


# the kernel mode of each objective (RH_GAN_* of include/rave_hip.h): how RAVE.training_step recognises them
hinge_gan.gan_mode, ls_gan.gan_mode, nonsaturating_gan.gan_mode = 0, 1, 2
GAN_LOSSES = {"hinge": hinge_gan, "ls": ls_gan, "nonsaturating": nonsaturating_gan}


class MultiScaleSTFT(nn.Module):
    """rave/core.py:269-319 without mel; torchaudio.transforms.Spectrogram(n_fft=s, win_length=s, hop_length=s//4,
    normalized, power=None) == torch.stft(periodic Hann, center, reflect) [/ sqrt(sum(window^2))].  ``normalized`` is folded
    into the ``window_<s>`` buffers (the transform is linear in the window), so every consumer of them sees it.
    ``magnitude=False``: ``forward`` returns the reference's ``stack([re, im], -1)``, (rows, bins, frames, 2) per scale, from
    the rave_amd.Spectrogram kernel (rave_amd/csrc/spectrogram.hip) where rh_spectrogram_supported holds and from torch.stft
    elsewhere (CPU tensors, other dtypes, unbuilt sizes)."""

    def __init__(self, scales: Sequence[int], sample_rate: int = 44100, magnitude: bool = True, normalized: bool = False,
                 num_mels=None):
        super().__init__()
        if num_mels is not None:
            raise NotImplementedError("rave_amd MultiScaleSTFT: num_mels is not built (the mel variant of the spectral losses is "
                                      "SpectralDistance(mel=...), rave_amd/configs/mi355x_encodec_mel.gin)")
        self.scales = list(scales)
        self.magnitude, self.normalized, self.num_mels = bool(magnitude), bool(normalized), None
        for s in self.scales:
            w = torch.hann_window(s)
            if self.normalized:
                w = (w.double() / w.double().pow(2).sum().sqrt()).float()
            self.register_buffer(f"window_{s}", w, persistent=False)

    def windows(self):
        return [getattr(self, f"window_{s}") for s in self.scales]

    def complex_stfts(self, x):
        """Complex spectrograms (rows, frames, bins): torch.stft's with the (frequency, frame) axes swapped."""
        x = x.reshape(-1, x.shape[-1])
        # framing (centre + reflect pad + Hann window) in one HIP pass (raises on a CPU tensor), FFT on rocFFT
        from . import ops
        return [torch.fft.rfft(ops.stft_frames(x, getattr(self, f"window_{s}"), s, s // 4), dim=-1) for s in self.scales]

    def forward(self, x):
        """Magnitudes in torch.stft's (rows, bins, frames) layout; with ``magnitude=False`` (rows, bins, frames, 2)."""
        if self.magnitude:
            return [y.abs().transpose(-1, -2) for y in self.complex_stfts(x)]
        from . import ops
        x = x.reshape(-1, x.shape[-1])
        # the window buffer carries the normalisation already: normalized=False below
        return [ops.spectrogram(x, w, s, s // 4, False, True).movedim(-3, -1) for s, w in zip(self.scales, self.windows())]


class AudioDistanceV1(nn.Module):
    """rave/core.py:322-344."""

    def __init__(self, multiscale_stft, log_epsilon: float) -> None:
        super().__init__()
        self.multiscale_stft = multiscale_stft()
        self.log_epsilon = log_epsilon

    def forward(self, x, y):
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError("rave_amd AudioDistanceV1: inputs must live on the GPU (the HIP path has no CPU fallback)")
        # STFT, magnitudes, both distances and their reductions inside one HIP kernel per scale (rh_stft_loss_*_f32)
        from . import ops
        ms = self.multiscale_stft
        xr, yr = x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1])
        # all scales in ONE autograd node: the scale sum and the per-signal gradient accumulation happen inside
        distance = ops.multiscale_stft_distance(xr, yr, [getattr(ms, f"window_{s}") for s in ms.scales], ms.scales,
                                                float(self.log_epsilon))
        return {"spectral_distance": distance}


class WeightedInstantaneousSpectralDistance(nn.Module):
    """rave/core.py:347-412: the amplitude distance with log1p, plus ``phase_distance``, the mean squared difference of the
    instantaneous frequencies (wrapped phase differences along the frames), optionally weighted by clip(log1p|X|, 0, 1) of the
    target.  ``multiscale_stft`` must build a ``MultiScaleSTFT(magnitude=False)``.

    f32 GPU signals at built scales run one HIP launch per scale and direction with the transform inside
    (rave_amd/csrc/inst_freq_loss.hip, ``ops.multiscale_inst_freq_distance``); CPU tensors, other dtypes and unbuilt scales run
    the reference's torch composition, cumsum included (``ops.inst_freq_compose``), and so does everything under
    ``RH_INST_FREQ=0``.  Bound by rave_amd/configs/mi355x_phase.gin; no shipped default selects it."""

    def __init__(self, multiscale_stft, weighted: bool = False) -> None:
        super().__init__()
        self.multiscale_stft = multiscale_stft()
        if getattr(self.multiscale_stft, "magnitude", False):
            raise ValueError("rave_amd WeightedInstantaneousSpectralDistance: needs MultiScaleSTFT(magnitude=False) (the "
                             "reference asserts a trailing (re, im) axis, rave/core.py:377)")
        self.weighted = weighted

    def forward(self, target, pred):
        from . import ops
        ms = self.multiscale_stft
        xr, yr = target.reshape(-1, target.shape[-1]), pred.reshape(-1, pred.shape[-1])
        fused = (xr.is_cuda and yr.is_cuda and xr.dtype == torch.float32 and yr.dtype == torch.float32 and ops.inst_freq_on()
                 and ops.inst_freq_supported(ms.scales, xr.shape[-1], xr.shape[0]))
        fn = ops.multiscale_inst_freq_distance if fused else ops.inst_freq_compose
        spectral_distance, phase_distance = fn(xr, yr, ms.windows(), ms.scales, bool(self.weighted))
        return {"spectral_distance": spectral_distance, "phase_distance": phase_distance}


# ---- the other distances of rave/core.py (:415-490); no shipped config selects them (v1 ... v3, discrete use AudioDistanceV1)
class WaveformDistance(nn.Module):
    """rave/core.py:433-440."""

    def __init__(self, norm: str) -> None:
        super().__init__()
        self.norm = norm

    def forward(self, x, y):
        return mean_difference(y, x, self.norm)


class SpectralDistance(nn.Module):
    """rave/core.py:446-490: the spectrum of both signals, then ``mean_difference(y, x, norm)`` summed over the norms.  Unused by
    the shipped configs (v1 ... v3, discrete use AudioDistanceV1); the Encodec-style loss binds it by gin
    (rave_amd/configs/mi355x_encodec.gin, and mi355x_encodec_mel.gin for the mel variant).

    Without ``mel``: torchaudio Spectrogram(n_fft, hop = n_fft / 4, power, normalized, center=False).  GPU float32 signals of
    equal shape on one device, ``power`` 1 or 2, ``norm`` "L1", "L2" or both, at a built size (n_fft a power of two in
    128 ... 2048, T >= n_fft: ``ops.spec_dist_supported``) run rave_amd/csrc/spec_dist.hip: the transform, ``|.|^power`` and both
    reductions in one launch forward and one backward, no spectrum in memory (``ops.multiscale_spec_distance``; an
    ``EncodecAudioDistance`` of such members runs all of its scales as one autograd node).  Everything else -- CPU tensors,
    other dtypes, ``power=None`` (a complex spectrum), n_fft 32 / 64, ``RH_SPEC_DIST=0`` -- runs the torch composition
    (``ops.spec_dist_compose``): a strided view, rocFFT, ATen reductions.

    ``mel=n``: torchaudio MelSpectrogram(sampling_rate, n_fft, hop = n_fft / 4, n_mels=n, power, normalized, center=False) as
    ``rave_amd.mel.DifferentiableMelSpectrogram`` (submodule ``mel_spec``, with torchaudio's two buffers): on GPU float32 signals
    one HIP launch forward and one backward per signal (rave_amd/csrc/mel.hip), the torch composition elsewhere.  The
    reductions stay ATen on the small mel tensors.  ``power`` must be 1 or 2 (torchaudio has no complex mel spectrogram)."""

    def __init__(self, n_fft: int, sampling_rate: int, norm, power, normalized: bool, mel=None) -> None:
        super().__init__()
        self.n_fft, self.hop, self.power, self.normalized = int(n_fft), int(n_fft) // 4, power, bool(normalized)
        if mel:
            if power is None:
                raise ValueError("rave_amd SpectralDistance: mel needs power 1 or 2, got power=None (a mel spectrogram of a "
                                 "complex spectrum is not defined; torchaudio refuses it as well)")
            from .mel import DifferentiableMelSpectrogram
            self.mel_spec = DifferentiableMelSpectrogram(int(sampling_rate), self.n_fft, hop_length=self.hop, n_mels=int(mel),
                                                         power=power, normalized=self.normalized, center=False, pad_mode=None)
        else:
            self.register_buffer("window", torch.hann_window(self.n_fft), persistent=False)
        self.norm = (norm,) if isinstance(norm, str) else tuple(norm)

    def spec(self, x: torch.Tensor) -> torch.Tensor:
        """(..., T) -> (..., n_fft / 2 + 1, frames), torch.stft(center=False) layout; with ``mel``: (..., n_mels, frames)."""
        if "mel_spec" in self._modules:                                 # (the plain variant has no such attribute at all)
            return self.mel_spec(x)
        from . import ops
        return ops.spec_dist_spectrum(x, self.window, self.n_fft, self.power, self.normalized)

    def is_plain(self) -> bool:
        return "mel_spec" not in self._modules

    def refresh_host_caches(self) -> None:
        """GraphedTrainingStep calls this before it records: the window's norm is read on the host here, outside the capture."""
        if self.is_plain() and self.normalized and self.window.is_cuda:
            from . import ops
            ops._spec_dist_scale(self.window)

    def forward(self, x, y):
        if self.is_plain():
            from . import ops
            if _spec_dist_kernel(x, y, [self]):
                return ops.multiscale_spec_distance(x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1]), [self.window],
                                                    [self.n_fft], self.norm, self.power, self.normalized)
            return ops.spec_dist_compose(x, y, self.window, self.n_fft, self.norm, self.power, self.normalized)
        x = self.spec(x)
        y = self.spec(y)
        distance = 0
        for norm in self.norm:
            distance = distance + mean_difference(y, x, norm)
        return distance


def _spec_dist_kernel(x, y, members) -> bool:
    """The plain ``SpectralDistance`` members (one, or all of an ``EncodecAudioDistance``) take the HIP kernels
    (rave_amd/csrc/spec_dist.hip) on float32 signals of equal shape on one GPU when they agree in ``power`` (1 or 2),
    ``normalized`` and ``norm`` ("L1", "L2" or both) and every scale is built; CPU tensors, other dtypes, unequal (broadcasting)
    shapes, anything else and ``RH_SPEC_DIST=0`` run the torch composition."""
    if not (torch.is_tensor(x) and torch.is_tensor(y) and x.is_cuda and y.is_cuda and x.dtype == torch.float32
            and y.dtype == torch.float32 and x.device == y.device and x.shape == y.shape and x.dim() >= 1 and x.numel() > 0):
        return False
    first = members[0]
    if not all(type(m) is SpectralDistance and m.is_plain() and m.power == first.power and m.normalized == first.normalized
               and m.norm == first.norm and m.window.device == x.device and m.window.dtype == torch.float32 for m in members):
        return False
    if first.power not in (1, 2) or sorted(first.norm) not in (["L1"], ["L2"], ["L1", "L2"]):
        return False
    from . import ops
    t = x.shape[-1]
    return ops.spec_dist_on() and ops.spec_dist_supported([m.n_fft for m in members], t, x.numel() // t, first.power)


class EncodecAudioDistance(nn.Module):
    """rave/core.py:415-431.  Plain ``SpectralDistance`` members that agree in ``power``, ``normalized`` and ``norm`` run all of
    their scales as ONE autograd node on the HIP kernels where every scale is built (``_spec_dist_kernel``); any other list
    runs member by member."""

    def __init__(self, scales, spectral_distance) -> None:
        super().__init__()
        self.waveform_distance = WaveformDistance(norm="L1")
        self.spectral_distances = nn.ModuleList([spectral_distance(scale) for scale in scales])

    def forward(self, x, y):
        waveform_distance = self.waveform_distance(x, y)
        members = list(self.spectral_distances)
        if members and _spec_dist_kernel(x, y, members):
            from . import ops
            first = members[0]
            spectral_distance = ops.multiscale_spec_distance(x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1]),
                                                             [m.window for m in members], [m.n_fft for m in members],
                                                             first.norm, first.power, first.normalized)
            return {"waveform_distance": waveform_distance, "spectral_distance": spectral_distance}
        spectral_distance = 0
        for dist in self.spectral_distances:
            spectral_distance = spectral_distance + dist(x, y)
        return {"waveform_distance": waveform_distance, "spectral_distance": spectral_distance}
