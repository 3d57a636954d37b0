"""CPU tests of the filtered-noise synthesis (csrc/noise_synth.hip): the two identities the kernel rests on against the float64
torch composition, the host side of its ABI (size query, the table), and the modules' unchanged behaviour on CPU tensors."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import noise_synth_reference as R


@pytest.mark.parametrize("nb,n", R.SIZES)
def test_direct_form_equals_the_composition(nb, n):
    """amp_to_impulse_response is the matrix ``table`` and fft_convolve a causal convolution cut to n, forward and backward, to
    1e-12 (float64; values of order 1)."""
    h, noise, gout = R.inputs(nb, n, d=3, t=5)
    want, want_gh = R.composition_with_grad(h, noise, gout, nb, n)
    m = R.table(nb, n)
    assert tuple(m.shape) == (n, nb)
    assert float((R.forward(h, noise, m) - want).abs().max()) <= 1e-12
    assert float((R.backward(h, noise, m, gout) - want_gh).abs().max()) <= 1e-12


@pytest.mark.parametrize("nb,n", R.SIZES)
def test_host_table_is_the_rounded_composition(nb, n):
    """rh_noise_synth_table_f32 (f64 on the host, rounded once) against ``table``: a correctly rounded float32 is within
    2^-24 |x| of x, and the two float64 evaluations differ by their own rounding (a few 1e-16 on values below 1: 2e-15)."""
    from rave_amd import ops
    got = ops.noise_synth_table(nb, n)
    want = R.table(nb, n)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, nb) and not got.is_cuda
    assert bool(((got.double() - want).abs() <= 2.0 ** -24 * want.abs() + 2e-15).all())
    assert float(want.abs().max()) > 1e-3


def test_supported_sizes():
    from rave_amd import _lib as L
    from rave_amd import ops
    for nb, n in R.SIZES + [(2, 1), (33, 1), (2, 64)]:
        assert L.lib.rh_noise_synth_supported(nb, n) == 1 and ops.noise_synth_supported(nb, n), (nb, n)
    for nb, n in [(34, 64), (1, 8), (5, 65), (5, 0), (0, 0), (-1, 8)]:
        assert L.lib.rh_noise_synth_supported(nb, n) == 0 and not ops.noise_synth_supported(nb, n), (nb, n)
    buf = (C.c_float * (65 * 5))()
    assert L.lib.rh_noise_synth_table_f32(5, 65, buf) == -2          # RH_ERR_UNSUPPORTED
    assert L.lib.rh_noise_synth_table_f32(5, 64, None) == -1         # RH_ERR_INVALID
    with pytest.raises(RuntimeError, match="noise_synth_table"):
        ops.noise_synth_table(34, 64)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Null pointers, non-positive extents and unbuilt sizes are answered on the host (no GPU is touched)."""
    from rave_amd import _lib as L
    p = 4096                                                         # any non-null address: nothing dereferences it
    assert L.lib.rh_noise_synth_fwd_f32(None, p, p, 1, 1, 1, 5, 8, p, None) == -1
    assert L.lib.rh_noise_synth_bwd_f32(p, p, p, p, 1, 1, 1, 5, 8, None, None) == -1
    assert L.lib.rh_noise_synth_fwd_f32(p, p, p, 0, 1, 1, 5, 8, p, None) == -1
    assert L.lib.rh_noise_synth_bwd_f32(p, p, p, p, 1, 1, 0, 5, 8, p, None) == -1
    assert L.lib.rh_noise_synth_fwd_f32(p, p, p, 1, 1, 1, 34, 8, p, None) == -2
    assert L.lib.rh_noise_synth_bwd_f32(p, p, p, p, 1, 1, 1, 5, 65, p, None) == -2
    assert b"noise_synth_bwd" in L.lib.rh_last_error()


def test_op_raises_on_cpu_and_non_f32_tensors():
    from rave_amd import ops
    h, noise, table = torch.zeros(1, 5, 2), torch.zeros(1, 2, 1, 8), ops.noise_synth_table(5, 8)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.noise_synth(h, noise, table, 5, 8)


class _Pass(nn.Module):
    """Stands in for the branch's convolutions (HIP only): the module's input IS the last convolution's output."""

    def forward(self, x, act=0, slope=0.2):
        return x


def _modules():
    from rave_amd import blocks
    return [(blocks.NoiseGenerator(in_size=8, data_size=4), 4, 5, 64),
            (blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 5, n_channels=2), 8, 5, 8),
            (blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 32), 4, 32, 8)]


def test_modules_on_cpu_tensors_run_the_composition():
    """CPU tensors take the reference's composition, bit for bit what it gave before the kernel existed, with injected noise
    and with the module's own draw."""
    for m, d, nb, n in _modules():
        m.net = nn.Sequential(_Pass())
        h64, noise64, _ = R.inputs(nb, n, d, t=3)
        h, noise = h64.float(), noise64.float()
        want = R.composition(h, noise, nb, n)
        assert torch.equal(m(h, noise=noise), want)
        assert float((want.double() - R.composition(h64, noise64, nb, n)).norm() / want.double().norm()) < 1e-5
        torch.manual_seed(3)
        got = m(h)
        torch.manual_seed(3)
        drawn = torch.rand(h.shape[0], 3, d, n) * 2 - 1
        assert torch.equal(got, R.composition(h, drawn, nb, n))


def test_state_dict_keys_are_unchanged_and_the_table_is_a_non_persistent_buffer():
    from rave_amd import blocks
    v1 = blocks.NoiseGenerator(in_size=8, data_size=4)
    v2 = blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 5, n_channels=2)
    for m in (v1, v2):
        assert set(m.state_dict()) == {"target_size", "net.0.weight", "net.2.weight", "net.4.weight"}
        m.load_state_dict(m.state_dict())                            # strict
    assert tuple(v1.noise_table.shape) == (64, 5) and tuple(v2.noise_table.shape) == (8, 5)
    assert dict(v1.named_buffers())["noise_table"] is v1.noise_table
    # an unbuilt size has no table: the module runs the composition wherever it lives
    assert blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 40).noise_table is None


def test_table_is_not_broadcast_every_step():
    """The table is a constant of (noise_bands, target_size): identical on every rank, like the PQMF filters."""
    from rave_amd import blocks
    from rave_amd.ddp import BufferSync
    m = blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 5)
    s = BufferSync(m)
    assert [id(b) for b in s.skipped] == [id(m.noise_table)] and [id(b) for b in s.ibufs] == [id(m.target_size)]
