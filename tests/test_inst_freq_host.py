"""CPU tests of the instantaneous-frequency distance: rave_amd.losses.WeightedInstantaneousSpectralDistance and
MultiScaleSTFT(magnitude=False) on CPU tensors (the torch composition) against tests/inst_freq_reference.py and, where the
reference tree is present, against the reference's own classes (rave/core.py:269-319, :347-412) on the oracle shims."""
from functools import partial

import pytest
import torch

import inst_freq_reference as R
from conftest import rel_l2

SCALES = [512, 256, 128]


def _signals():
    g = torch.Generator().manual_seed(0)
    x = 0.3 * torch.randn(2, 1, 3000, generator=g)
    y = 0.5 * x + 0.2 * torch.randn(2, 1, 3000, generator=g)
    return x, y


def _run(dist, x, y, w=(1.0, 0.37)):
    x = x.clone().requires_grad_(True)
    y = y.clone().requires_grad_(True)
    out = dist(x, y)
    out = dict(out)
    (w[0] * out["spectral_distance"] + w[1] * out["phase_distance"]).backward()
    return {k: v.detach() for k, v in out.items()}, x.grad, y.grad


def _restated(x, y, normalized, weighted, dtype, w=(1.0, 0.37)):
    x = x.to(dtype).detach().clone().requires_grad_(True)
    y = y.to(dtype).detach().clone().requires_grad_(True)
    sd, pd, _ = R.distance(x, y, SCALES, normalized, weighted, dtype)
    (w[0] * sd + w[1] * pd).backward()
    return dict(spectral_distance=sd.detach(), phase_distance=pd.detach()), x.grad, y.grad


def _ours(normalized, weighted):
    from rave_amd import losses
    return losses.WeightedInstantaneousSpectralDistance(
        partial(losses.MultiScaleSTFT, scales=SCALES, sample_rate=44100, magnitude=False, normalized=normalized), weighted=weighted)


def _reference_core():
    from ref_import import import_reference, reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    import_reference()
    import rave.core as core
    return core


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("normalized", [True, False])
def test_cpu_class_equals_the_restatement(normalized, weighted):
    """The CPU path of the class is the literal composition: same values and gradients as the f32 restatement up to the
    rounding of the window normalisation (folded into the window here, applied after the transform there), judged against the
    f64 restatement: no further from it than 4 x the f32 restatement itself (floor 1e-5)."""
    x, y = _signals()
    out, gx, gy = _run(_ours(normalized, weighted), x, y)
    assert set(out) == {"spectral_distance", "phase_distance"}
    o32, gx32, gy32 = _restated(x, y, normalized, weighted, torch.float32)
    o64, gx64, gy64 = _restated(x, y, normalized, weighted, torch.float64)
    for k in o64:
        err = abs(float(out[k]) - float(o64[k])) / abs(float(o64[k]))
        assert err <= max(1e-5, 4 * abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))), (k, err)
    for mine, r32, r64 in ((gx, gx32, gx64), (gy, gy32, gy64)):
        assert mine.shape == x.shape
        assert rel_l2(mine, r64) <= max(1e-5, 4 * rel_l2(r32, r64)), (rel_l2(mine, r64), rel_l2(r32, r64))


@pytest.mark.parametrize("weighted", [False, True])
def test_class_and_restatement_equal_the_reference_class(weighted):
    """The reference's own WeightedInstantaneousSpectralDistance over its MultiScaleSTFT(magnitude=False, normalized=True) on
    the torchaudio shim: its values and gradients, the f32 restatement's and the class's agree to f32 rounding (each judged
    against the f64 restatement, 4 x the reference's own error, floor 1e-5)."""
    core = _reference_core()
    x, y = _signals()
    ref = core.WeightedInstantaneousSpectralDistance(
        partial(core.MultiScaleSTFT, scales=SCALES, sample_rate=44100, magnitude=False, normalized=True), weighted=weighted)
    outr, gxr, gyr = _run(ref, x, y)
    out, gx, gy = _run(_ours(True, weighted), x, y)
    o32, gx32, gy32 = _restated(x, y, True, weighted, torch.float32)
    o64, gx64, gy64 = _restated(x, y, True, weighted, torch.float64)
    assert set(outr) == set(out) == {"spectral_distance", "phase_distance"}
    for k in o64:
        want = abs(float(o64[k]))
        bound = max(1e-5, 4 * abs(float(outr[k]) - float(o64[k])) / want)
        assert abs(float(outr[k]) - float(o64[k])) / want <= 1e-4, k        # the restatement states the reference
        assert abs(float(out[k]) - float(o64[k])) / want <= bound, k
        assert abs(float(o32[k]) - float(o64[k])) / want <= bound, k
    for mine, r32, rr, r64 in ((gx, gx32, gxr, gx64), (gy, gy32, gyr, gy64)):
        bound = max(1e-5, 4 * rel_l2(rr, r64))
        assert rel_l2(rr, r64) <= 1e-2
        assert rel_l2(mine, r64) <= bound and rel_l2(r32, r64) <= bound, (rel_l2(mine, r64), rel_l2(r32, r64), bound)


@pytest.mark.parametrize("normalized", [True, False])
def test_multiscale_stft_complex_output_equals_the_reference(normalized):
    """MultiScaleSTFT(magnitude=False): (rows, bins, frames, 2) per scale, the restatement's values."""
    from rave_amd import losses
    x, _ = _signals()
    x = x.reshape(1, 2, -1)                                  # (b, c, t) -> rows = b c
    ms = losses.MultiScaleSTFT(SCALES, 44100, magnitude=False, normalized=normalized)
    outs = ms(x)
    assert len(outs) == len(SCALES)
    for n, o in zip(SCALES, outs):
        want = torch.view_as_real(R.stft(x.reshape(2, -1).double(), n, normalized))
        assert tuple(o.shape) == (2, n // 2 + 1, 3000 // (n // 4) + 1, 2) == tuple(want.shape)
        assert rel_l2(o, want) <= 2e-6
    with pytest.raises(NotImplementedError, match="num_mels"):
        losses.MultiScaleSTFT(SCALES, 44100, magnitude=False, num_mels=64)


@pytest.mark.parametrize("normalized", [True, False])
def test_multiscale_stft_complex_output_equals_the_reference_module(normalized):
    from rave_amd import losses
    core = _reference_core()
    x = _signals()[0].reshape(1, 2, -1)
    outs = losses.MultiScaleSTFT(SCALES, 44100, magnitude=False, normalized=normalized)(x)
    for o, r in zip(outs, core.MultiScaleSTFT(SCALES, 44100, magnitude=False, normalized=normalized)(x)):
        assert o.shape == r.shape and rel_l2(o, r) <= 2e-6


def test_the_loss_refuses_a_magnitude_stft():
    from rave_amd import losses
    with pytest.raises(ValueError, match="magnitude=False"):
        losses.WeightedInstantaneousSpectralDistance(partial(losses.MultiScaleSTFT, scales=SCALES, sample_rate=44100))
