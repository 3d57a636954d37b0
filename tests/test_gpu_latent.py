"""Latent-space analysis and receptive field at the end of validation, on the GPU: the moment kernel
(rave_amd/csrc/latent_stats.hip) through the C ABI against numpy in float64, and ``RAVE.validation_epoch_end`` against what the
reference's own left behind (tests/golden/latent_tiny.pt, tools/make_golden_latent.py).

Moments: every entry within n * 2^-52 of numpy's, relative -- the bound for two float64 summations of the same n exact
products in different orders (each within (n - 1) * 2^-53 of the true sum, relative to the sum of the terms' magnitudes).  The
inputs are s_c * (1 + g / 8), s_c = +-1 per channel, g normal: all terms of one entry have one sign (|g| < 8), so that sum of
magnitudes IS the entry and the bound is a relative one per entry, as stated.
Analysis: no farther from the float64 restatement than the reference is (``ref_err`` in the fixture: 3.7e-8 / 5.0e-8 / 8.7e-13
for mean / fidelity / component direction at 8 channels)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import latent_cases as LC
import rave_oracle as O

pytestmark = pytest.mark.gpu

#          B, C,   T
SHAPES = [(1, 5, 1),          # one row
          (3, 8, 5),          # the tiny model's channel count, odd B and T
          (2, 128, 37),       # the largest channel count: every 32-channel tile full
          (4, 33, 130)]       # one channel into the second tile; T across two 64-step chunks and a ragged third
N_CALLS = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def batches(shape, seed=0):
    b, c, t = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0).view(1, c, 1)
    out = [sign * (1.0 + torch.randn(b, c, t, generator=gen) / 8) for _ in range(N_CALLS)]
    assert all(bool((z * sign > 0).all()) for z in out)
    return out


_REF = {}


def numpy_moments(shape):
    """count, sum[C], outer[C, C] of the three batches together, numpy float64 (computed once per shape)."""
    if shape not in _REF:
        c = shape[1]
        z = np.concatenate([m.numpy().astype(np.float64).transpose(0, 2, 1).reshape(-1, c) for m in batches(shape)], 0)
        _REF[shape] = (z.shape[0], z.sum(0), z.T @ z)
    return _REF[shape]


def workspace(shape, dev):
    from rave_amd import _lib as L
    n = C.c_int64(0)
    L.check(L.lib.rh_latent_moments_workspace_bytes(*shape, C.byref(n)), "workspace_bytes")
    assert n.value > 0 and n.value % 8 == 0
    return torch.empty(n.value // 8, dtype=torch.float64, device=dev)


def accumulate(shape, dev, means=None, acc=None):
    """Three calls of the entry point on one accumulator."""
    from rave_amd import _lib as L
    c = shape[1]
    if acc is None:
        acc = torch.zeros(1 + c + c * c, dtype=torch.float64, device=dev)
    ws = workspace(shape, dev)
    for m in (means if means is not None else [m.to(dev) for m in batches(shape)]):
        L.check(L.lib.rh_latent_moments_acc_f64(L.ptr(m), *shape, L.ptr(acc), L.ptr(ws), L.stream()), "latent_moments_acc")
    torch.cuda.synchronize()
    return acc


def check_moments(acc, shape):
    n, s, outer = numpy_moments(shape)
    c = shape[1]
    got = acc.cpu().numpy()
    assert got[0] == n == N_CALLS * shape[0] * shape[2]
    bound = n * 2.0 ** -52
    err_s = np.abs(got[1:1 + c] - s) / np.abs(s)
    err_o = np.abs(got[1 + c:].reshape(c, c) - outer) / np.abs(outer)
    print(f"{shape}: n = {n}, relative error sum {err_s.max():.2e} outer {err_o.max():.2e}, bound {bound:.2e}")
    assert err_s.max() <= bound and err_o.max() <= bound


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_moments_against_numpy_f64(dev, shape):
    acc = accumulate(shape, dev)
    check_moments(acc, shape)
    outer = acc[1 + shape[1]:].reshape(shape[1], shape[1])
    assert torch.equal(outer, outer.T)                    # both triangles are computed, by the same sums
    assert torch.equal(accumulate(shape, dev), acc)       # the same calls again: the same bits


def test_moments_at_a_4_byte_aligned_pointer(dev):
    """``mean`` at every residue of its address modulo 16, the accumulator 8-byte aligned only: same bits, nothing written
    outside the accumulator."""
    from misaligned import carve, guards_intact
    shape = (4, 33, 130)
    c = shape[1]
    want = accumulate(shape, dev)
    for off in (1, 2, 3):
        means = [carve(m.to(dev), off) for m in batches(shape)]
        acc = carve(torch.zeros(1 + c + c * c, dtype=torch.float64, device=dev), 2)
        assert means[0].data_ptr() % 16 == 4 * off and acc.data_ptr() % 16 == 8
        accumulate(shape, dev, means, acc)
        assert torch.equal(acc, want), off
        assert guards_intact(acc) and all(guards_intact(m) for m in means)
    check_moments(want, shape)


def test_unsupported_sizes_are_refused(dev):
    from rave_amd import _lib as L
    assert L.lib.rh_latent_moments_supported(128) == 1 and L.lib.rh_latent_moments_supported(1) == 1
    assert L.lib.rh_latent_moments_supported(129) == 0 and L.lib.rh_latent_moments_supported(0) == 0
    z = torch.ones(2, 129, 4, device=dev)
    acc = torch.zeros(1 + 129 + 129 * 129, dtype=torch.float64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=dev)
    n = C.c_int64(0)
    invalid = -1                                          # RH_ERR_INVALID
    assert L.lib.rh_latent_moments_workspace_bytes(2, 129, 4, C.byref(n)) == invalid
    assert L.lib.rh_latent_moments_workspace_bytes(2, 8, 4, None) == invalid
    run = L.lib.rh_latent_moments_acc_f64
    assert run(L.ptr(z), 2, 129, 4, L.ptr(acc), L.ptr(ws), L.stream()) == invalid
    for bad in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (-1, 8, 4)):
        assert run(L.ptr(z), *bad, L.ptr(acc), L.ptr(ws), L.stream()) == invalid, bad
    for args in ((None, L.ptr(acc), L.ptr(ws)), (L.ptr(z), None, L.ptr(ws)), (L.ptr(z), L.ptr(acc), None)):
        assert run(args[0], 2, 8, 4, args[1], args[2], L.stream()) == invalid
    torch.cuda.synchronize()
    assert not bool(acc.any())                            # nothing was enqueued


def test_latent_analysis_update_on_the_device(dev):
    """rave_amd.latent.LatentAnalysis: the device path is the kernel (same accumulator as the C ABI gives), the wide fixture
    through it is as close to float64 as the reference."""
    from rave_amd.latent import LatentAnalysis
    shape = (3, 8, 5)
    la = LatentAnalysis()
    for m in batches(shape):
        la.update(m.to(dev))
    assert la.acc.is_cuda and torch.equal(la.acc, accumulate(shape, dev))
    rec = LC.golden()["wide"]
    la = LatentAnalysis()
    for _, mean in LC.out_list(rec, dev):
        la.update(mean)
    mean, pca, fid = la.finish()
    LC.check_against_fixture(mean, pca, fid, rec)
    assert LC.fidelity_p(fid) == rec["fidelity_p"]


def tiny_model(dev, causal, latent_analysis=True):
    from rave_amd import model as M
    g = LC.golden()
    m = M.build_v2(causal=causal, latent_analysis=latent_analysis, **g["config"])
    sd = {k: v for k, v in LC.fixture_state_dict(g).items() if k not in LC.ANALYSIS_KEYS + ("receptive_field",)}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= set(LC.ANALYSIS_KEYS) | {"receptive_field"}
    return m.to(dev).train()


N_SIGNAL = 2 ** 17      # 8192 band samples: the crop by either fixture's receptive field leaves more than the largest STFT window


@pytest.mark.parametrize("tag,causal", [("tiny", False), ("tiny_causal", True)])
def test_validation_epoch_end_against_the_reference(dev, tag, causal):
    g = LC.golden()
    rec = g[tag]
    m = tiny_model(dev, causal)
    env = {k: os.environ.get(k) for k in ("RH_CONV_X6", "RH_WGRAD_X6")}
    m.validation_epoch_end(LC.out_list(g["tiny"], dev))
    # what the probe borrowed is back
    assert m.training and all(mod.training for mod in m.modules())
    assert {k: os.environ.get(k) for k in env} == env
    assert all(p.grad is None for p in m.parameters())
    assert all(getattr(mod, "_prepacked", None) is None for mod in m.modules())
    print(tag, "receptive field", m.receptive_field.tolist(), "reference", rec["receptive_field"].tolist())
    assert m.receptive_field.tolist() == rec["receptive_field"].tolist()
    LC.check_against_fixture(m.latent_mean, m.latent_pca, m.fidelity, g["tiny"])
    assert {str(p): m.logged[f"fidelity_{p}"] for p in LC.PERCENT} == rec["fidelity_p"]
    # the next training step crops by the new field
    m.configure_optimizers()
    logged = m.training_step(O.synthetic_batch(1, 1, N_SIGNAL).to(dev), 0)
    assert m._rf_host == tuple(rec["receptive_field"].tolist())
    assert all(bool(torch.isfinite(v.detach()).all()) for v in logged.values() if torch.is_tensor(v))


def test_off_by_default_still_measures_the_receptive_field(dev):
    m = tiny_model(dev, False, latent_analysis=False)
    keys = set(m.state_dict())
    m.validation_epoch_end(LC.out_list(LC.golden()["tiny"], dev))
    assert m.receptive_field.tolist() == LC.golden()["tiny"]["receptive_field"].tolist()
    assert set(m.state_dict()) == keys and not any(k.startswith("fidelity") for k in m.logged)


def test_validation_epoch_end_to_end(dev):
    """training_step, validation_step x 2, validation_epoch_end, training_step on the tiny model: the cached receptive field
    is refreshed, the fidelity is a cumulative share and the components are orthonormal.  Orthonormality to 1e-5: the
    eigenvectors are orthonormal in float64, the cast of (at most) 128 unit rows to float32 costs <= 128 * 2^-24 ~ 8e-6 per
    entry of the product."""
    m = tiny_model(dev, False)
    m.configure_optimizers()
    x = O.synthetic_batch(2, 1, N_SIGNAL).to(dev)
    m.training_step(x[:1].clone(), 0)
    assert m._rf_host == (0, 0)
    m.eval()
    with torch.no_grad():
        out = [m.validation_step(x[i:i + 1], i) for i in range(2)]
    m.train()
    assert out[0][1].shape == (1, 8, N_SIGNAL // 2048)
    m.validation_epoch_end(out)
    rf = tuple(m.receptive_field.tolist())
    assert rf[0] > 0 and "validation" in m.logged and "fidelity_0.95" in m.logged
    m.training_step(x[:1].clone(), 1)
    assert m._rf_host == rf
    fid = m.fidelity.cpu()
    assert bool((fid[1:] >= fid[:-1]).all()) and float(fid[0]) > 0
    assert abs(float(fid[-1]) - 1.0) <= 2.0 ** -23
    pca = m.latent_pca.double().cpu()
    assert float((pca @ pca.T - torch.eye(8, dtype=torch.float64)).abs().max()) <= 1e-5
    z = torch.cat([mean.double().permute(0, 2, 1).reshape(-1, 8) for _, mean in out], 0).cpu()
    assert float((m.latent_mean.double().cpu() - z.mean(0)).abs().max()) <= 2.0 ** -23 * float(z.mean(0).abs().max()) + 1e-12
