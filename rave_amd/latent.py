"""Latent-space analysis at the end of validation (rave/model.py:463-488): mean, principal components and cumulative explained
variance ("fidelity") of the posterior means over the validation set.

The reference concatenates the epoch's latents, copies them to the host and runs sklearn's PCA on the (rows, channels) matrix.
Here the epoch is reduced to its first and second moments as it goes -- one call of rh_latent_moments_acc_f64 per validation
batch (csrc/latent_stats.hip: f64, one summation order, the (batch, channels, time) layout read in place) -- and ``finish``
takes the C x C covariance to the host once for a symmetric eigendecomposition in f64 (host-side plumbing: 128 x 128 at most).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

Tensor = torch.Tensor


class LatentAnalysis:
    """``update(mean)`` once per validation batch, then ``finish()``.  The accumulator (``acc``: count, sum[C], outer[C * C] in
    f64) lives where the first batch lives."""

    def __init__(self):
        self.acc: Optional[Tensor] = None
        self.channels = 0
        self._ws: Optional[Tensor] = None

    def update(self, mean: Tensor) -> None:
        if mean.dim() != 3 or mean.dtype != torch.float32:
            raise ValueError(f"LatentAnalysis.update: expected a float32 (batch, channels, time) tensor, got {tuple(mean.shape)} {mean.dtype}")
        b, c, t = mean.shape
        if self.acc is None:
            self.channels = c
            self.acc = torch.zeros(1 + c + c * c, dtype=torch.float64, device=mean.device)
        if c != self.channels or mean.device != self.acc.device:
            raise ValueError(f"LatentAnalysis.update: {c} channels on {mean.device}, the accumulator holds {self.channels} on {self.acc.device}")
        if b * t == 0:
            return
        mean = mean.detach()
        if mean.is_cuda:
            from . import _lib as L
            mean = mean.contiguous()
            nbytes = C.c_int64(0)
            L.check(L.lib.rh_latent_moments_workspace_bytes(b, c, t, C.byref(nbytes)), "latent_moments_workspace_bytes")
            if self._ws is None or self._ws.numel() * 8 < nbytes.value:
                self._ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=mean.device)
            with torch.cuda.device(mean.device):
                L.check(L.lib.rh_latent_moments_acc_f64(L.ptr(mean), b, c, t, L.ptr(self.acc), L.ptr(self._ws), L.stream()),
                        "latent_moments_acc")
        else:
            z = mean.double().permute(0, 2, 1).reshape(-1, c)      # "b c t -> (b t) c"
            self.acc[0] += b * t
            self.acc[1:1 + c] += z.sum(0)
            self.acc[1 + c:] += (z.T @ z).reshape(-1)

    def finish(self) -> Optional[Tuple[Tensor, Tensor, Tensor]]:
        """(latent_mean (C), components (C, C), fidelity (C)) as f32 host tensors; None when nothing was fed.  ``components[i]``
        is the eigenvector of the i-th largest eigenvalue of the sample covariance, as a row, its entry of largest magnitude
        positive (sklearn's svd_flip on the rows of V, which the reference's PCA applies); ``fidelity`` the cumulative
        eigenvalue share.  Fewer rows than channels raises, as sklearn's PCA refuses n_components > n_samples."""
        if self.acc is None:
            return None
        acc = self.acc.cpu()                                       # the one device-to-host copy of the epoch
        c = self.channels
        n = int(acc[0].item())
        if n == 0:
            return None
        if n < c:
            raise ValueError(f"LatentAnalysis.finish: {n} rows for {c} latent channels (the PCA needs at least as many rows as channels)")
        mu = acc[1:1 + c] / n
        outer = acc[1 + c:].reshape(c, c)
        cov = (outer - n * torch.outer(mu, mu)) / max(n - 1, 1)
        cov = 0.5 * (cov + cov.T)
        lam, vec = torch.linalg.eigh(cov)                          # ascending
        lam = lam.flip(0).clamp_min(0.0)
        comp = vec.flip(1).T.contiguous()                          # rows, descending
        pick = comp.abs().argmax(1, keepdim=True)
        comp = comp * torch.sign(comp.gather(1, pick))
        fidelity = torch.cumsum(lam / lam.sum(), 0)
        return mu.float(), comp.float(), fidelity.float()
