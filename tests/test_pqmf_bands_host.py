"""PQMF with 2, 4, 8 and 32 bands (the ``N_BAND`` macro of configs/v1.gin rebound), host side: the buffers the modules
design, their state_dict, and what the C ABI accepts.  tests/golden/pqmf_bands.pt holds the unmodified reference's
``CachedPQMF(100, M)`` (tools/make_golden_pqmf_bands.py)."""
import os

import pytest
import torch

BANDS = (2, 4, 8, 32)
SUPPORTED = (2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(os.path.join(golden_dir, "pqmf_bands.pt"), weights_only=False)


@pytest.fixture(scope="module")
def L():
    from rave_amd import _lib
    return _lib


@pytest.mark.parametrize("m", BANDS)
def test_designed_buffers_equal_the_reference(golden, m):
    from rave_amd import pqmf as P
    g = golden[m]
    q = P.CachedPQMF(100, m)
    assert torch.equal(q.h, g["h"]) and torch.equal(q.hk, g["hk"])
    assert torch.equal(q.forward_conv.weight.detach(), g["w_fwd"])
    assert torch.equal(q.inverse_conv.weight.detach(), g["w_inv"])
    sd = {k: tuple(v.shape) for k, v in q.state_dict().items()}
    assert sd == {"hk": (m, 32 * m), "h": tuple(g["h"].shape), "forward_conv.weight": (m, 1, 32 * m + 1),
                  "inverse_conv.weight": (m, m, 33)}
    assert q.forward_conv._pad == (16 * m, 16 * m) and q.inverse_conv._pad == (16, 16)
    n = P.PQMF(100, m, polyphase=False)
    assert set(n.state_dict().keys()) == {"hk", "h"} and torch.equal(n.hk, g["hk"])
    assert torch.equal(n._w_fwd, g["w_fwd"]) and torch.equal(n._w_inv, g["w_inv"])
    assert q._fold(q.forward_conv.weight) is None          # the folded fast form is the 16-band bank's only


def test_prototype_lengths(golden):
    assert {m: golden[m]["h"].numel() for m in BANDS} == {2: 49, 4: 95, 8: 189, 32: 753}


def test_supported_query(L):
    for m in range(-2, 130):
        assert bool(L.lib.rh_pqmf_supported(m, 32 * m + 1)) == (m in SUPPORTED), m
    for m in SUPPORTED:
        # the kernel length is an input: anything the launcher can stage (<= 40 polyphase taps), not only the designed one
        assert L.lib.rh_pqmf_supported(m, 1) and L.lib.rh_pqmf_supported(m, 40 * m)
        assert not L.lib.rh_pqmf_supported(m, 0) and not L.lib.rh_pqmf_supported(m, -5)
        assert not L.lib.rh_pqmf_supported(m, 40 * m + 1)
        assert L.lib.rh_pqmf_tile_frames(m) > 0
    assert L.lib.rh_pqmf_tile_frames(3) == 0


def _entry_points(L):
    return (L.lib.rh_pqmf_analysis_fwd_f32, L.lib.rh_pqmf_analysis_bwd_f32, L.lib.rh_pqmf_synthesis_fwd_f32,
            L.lib.rh_pqmf_synthesis_bwd_f32)


@pytest.mark.parametrize("m", [3, 64, 0])
def test_entry_points_refuse_other_band_counts(L, m):
    for f in _entry_points(L):
        assert f(None, None, 0, 64, m, 33, 16, 4, None, None) == -2          # RH_ERR_UNSUPPORTED
        msg = L.lib.rh_last_error().decode()
        assert "2, 4, 8, 16, 32" in msg and str(m) in msg, msg


@pytest.mark.parametrize("m", SUPPORTED)
def test_entry_points_refuse_a_malformed_kernel(L, m):
    """Zero, negative, or more taps than the launcher stages: refused for every band count as for 16 (rows == 0, so that
    nothing is launched where the call is accepted)."""
    for f in _entry_points(L)[::3]:                        # analysis forward (kernel of 32 M + 1) and synthesis backward (33)
        for k in (0, -1, 41 * m):
            assert f(None, None, 0, 64 * m, m, k, 0, 64, None, None) == -2, (m, k)
            assert "kernel" in L.lib.rh_last_error().decode()
    assert L.lib.rh_pqmf_analysis_fwd_f32(None, None, 0, 64 * m, m, 32 * m + 1, 16 * m, 64, None, None) == 0
    assert L.lib.rh_pqmf_synthesis_fwd_f32(None, None, 0, 64, m, 41, 16, 56, None, None) == -2


def test_modules_refuse_other_band_counts():
    from rave_amd import pqmf as P
    for cls in (P.CachedPQMF, P.PQMF):
        with pytest.raises(NotImplementedError, match="1, 2, 4, 8, 16, 32"):
            cls(100, 64)
        with pytest.raises(AssertionError, match="power of 2"):       # the reference's own check (rave/pqmf.py:203-206)
            cls(100, 12, polyphase=True)
    with pytest.raises(NotImplementedError, match="1, 2, 4, 8, 16, 32"):
        P.PQMF(100, 12, polyphase=False)
    assert P.CachedPQMF(100, 1).n_band == 1                # the raw-waveform pass-through stays


def test_noncached_inverse_pads_reproduce_the_reference_forms(golden):
    """The pad pair (L/2 - 1, L/2 + 1) = (15, 17) that PQMF.inverse hands the synthesis kernel, derived in its docstring,
    against the oracle's polyphase and classic inverse on the CPU: for every M they are CachedPQMF.inverse's convolution
    with that pair."""
    import torch.nn.functional as F
    import rave_oracle as O
    for m in BANDS:
        g = golden[m]
        y = g["cot_y"]
        z = F.pad(O.reverse_half(y), (15, 17))
        x = F.conv1d(z, g["w_inv"]) * m
        x = x.flip(1).permute(0, 2, 1).reshape(y.shape[0], 1, -1)
        for ref in (O.pqmf_polyphase_inverse(y, g["hk"]), O.pqmf_classic_inverse(y, g["hk"])):
            assert ref.shape == x.shape
            assert float((x - ref).norm() / ref.norm()) < 2e-6, m
