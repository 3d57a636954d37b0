"""float64 yardsticks of the filtered-noise synthesis (a plain helper module, no fixtures).

``composition`` is the statement of rave/blocks.py:230-240, 282-292 in the functions rave_amd.blocks keeps for it (mod_sigmoid,
amp_to_impulse_response on torch.fft, fft_convolve, the two permutes), run in the dtype of its inputs: float64 inputs make it the
yardstick of every test, float32 inputs give the composition's own rounding error.  ``table``, ``forward`` and ``backward`` are
the direct form csrc/noise_synth.hip computes -- a matrix, a causal convolution, and their transposes -- so that the two
identities behind the kernel are themselves checked against the composition (tests/test_noise_synth_host.py).
"""
import torch

from rave_amd.blocks import amp_to_impulse_response, fft_convolve, mod_sigmoid

# (noise_bands, target_size): v1.gin, v2_small.gin (62-tap filter cropped to 8), noise.gin, the smallest, odd band counts, the
# largest built size, an odd target size below the filter length
SIZES = [(5, 64), (32, 8), (5, 8), (2, 4), (3, 4), (17, 32), (33, 64), (5, 3)]


def composition(h, noise, nb, n):
    """h (B, D nb, T), noise (B, T, D, n) -> (B, D, T n)."""
    amp = mod_sigmoid(h - 5).permute(0, 2, 1)
    amp = amp.reshape(amp.shape[0], amp.shape[1], -1, nb)
    out = fft_convolve(noise, amp_to_impulse_response(amp, n)).permute(0, 2, 1, 3)
    return out.reshape(out.shape[0], out.shape[1], -1)


def table(nb, n):
    """amp_to_impulse_response as its (n, nb) matrix: the composition applied to the identity, float64."""
    return amp_to_impulse_response(torch.eye(nb, dtype=torch.float64), n).t().contiguous()


def _lower(v):
    """(..., n) -> (..., n, n) with [i, k] = v[i - k] for k <= i and 0 above the diagonal."""
    n = v.shape[-1]
    lag = torch.arange(n)[:, None] - torch.arange(n)[None, :]
    return v[..., lag.clamp(min=0)] * (lag >= 0).to(v.dtype)


def forward(h, noise, m):
    """out[b, d, t n + i] = sum_{k <= i} noise[b, t, d, k] ir[i - k],  ir = m amp,  amp = 2 sigmoid(h - 5)^2.3 + 1e-7."""
    n, nb = m.shape
    amp = (2 * torch.sigmoid(h - 5) ** 2.3 + 1e-7).permute(0, 2, 1)
    amp = amp.reshape(amp.shape[0], amp.shape[1], -1, nb)
    out = torch.einsum("btdik,btdk->btdi", _lower(amp @ m.t()), noise).permute(0, 2, 1, 3)
    return out.reshape(out.shape[0], out.shape[1], -1)


def backward(h, noise, m, gout):
    """gh: d_ir[j] = sum_{i >= j} gout[i] noise[i - j],  d_amp = m^T d_ir,  gh = d_amp 4.6 s^2.3 (1 - s)."""
    n, nb = m.shape
    b, c, t = h.shape
    g = gout.reshape(b, c // nb, t, n).permute(0, 2, 1, 3)
    d_amp = torch.einsum("btdi,btdij->btdj", g, _lower(noise)) @ m
    s = torch.sigmoid(h - 5)
    return d_amp.reshape(b, t, c).permute(0, 2, 1) * 4.6 * s ** 2.3 * (1 - s)


def inputs(nb, n, d, t, batch=2, seed=0):
    """float64 (h, noise, gout): h uniform in [-12, 12] -- h - 5 from -17, where the 1e-7 floor of mod_sigmoid is all that is
    left, to 7, where the sigmoid is saturated --, noise uniform in [-1, 1), gout standard normal."""
    gen = torch.Generator().manual_seed(1000 * nb + 10 * n + seed)
    h = torch.rand(batch, d * nb, t, generator=gen, dtype=torch.float64) * 24 - 12
    noise = torch.rand(batch, t, d, n, generator=gen, dtype=torch.float64) * 2 - 1
    gout = torch.randn(batch, d, t * n, generator=gen, dtype=torch.float64)
    return h, noise, gout


def composition_with_grad(h, noise, gout, nb, n):
    """(out, gh) of the composition by autograd, in the inputs' dtype."""
    h = h.detach().clone().requires_grad_(True)
    out = composition(h, noise, nb, n)
    (gh,) = torch.autograd.grad(out, h, gout)
    return out.detach(), gh
