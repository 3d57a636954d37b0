"""Host-side premises of the misaligned-pointer tests (no GPU): the helper really produces the address residues and detects
overruns, and a data-parallel gradient bucket really hands the backward kernels pointers that are only 4-byte aligned."""
from functools import partial

import pytest
import torch

from misaligned import carve, guards_intact, residues


@pytest.mark.parametrize("dtype,offs", [(torch.float32, (0, 1, 2, 3)), (torch.int16, (0, 1, 2, 3)), (torch.int32, (0, 1, 2, 3)),
                                        (torch.int64, (0, 2)), (torch.float64, (0, 2))])
def test_carve_yields_the_requested_residue_and_keeps_the_values(dtype, offs):
    for n in (1, 5, 64, 1001):
        t = (torch.arange(n * 3, dtype=torch.float64).reshape(n, 3) - 7).to(dtype)
        for off in offs:
            v = carve(t, off)
            assert v.data_ptr() % 16 == 4 * off and v.is_contiguous() and v.shape == t.shape and v.dtype == dtype
            assert torch.equal(v, t)
            assert guards_intact(v)
            v.mul_(2)                      # writing INSIDE the view leaves the guards alone
            assert guards_intact(v) and torch.equal(v, t * 2)


def test_carve_refuses_a_residue_the_type_cannot_take():
    with pytest.raises(AssertionError):
        carve(torch.zeros(4, dtype=torch.int64), 1)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_guards_detect_a_one_element_overrun_on_either_side(off):
    t = torch.randn(7, 5)
    for where in ("before", "after"):
        v = carve(t, off)
        buf, start, n = v._carved
        assert guards_intact(v)
        buf[start - 1 if where == "before" else start + n] = 0.0
        assert not guards_intact(v), where
    # a NaN written over the (NaN) guard is an overrun too, unless it has the guard's own bits
    v = carve(t, off)
    buf, start, n = v._carved
    buf.view(torch.int32)[start + n] = 0x7FC00001
    assert not guards_intact(v)
    # the guards are quiet NaNs: whatever reads one is poisoned
    assert torch.isnan(buf[:start]).all() and torch.isnan(buf[start + n:]).all()
    # a tensor derived from the view (another object at the same address) is checked through the view's record
    v = carve(t, off)
    p = torch.nn.Parameter(v)
    assert guards_intact(p.data) and guards_intact(v.detach()) and guards_intact(v.view(-1))
    v._carved[0][v._carved[1] - 1] = 1.0
    assert not guards_intact(p.data)


def _v2_discriminator():
    from rave_amd import model as M
    return M.build_v2(capacity=16, latent_size=16).discriminator


def _spectral_discriminator():
    from rave_amd import discriminator as D
    return D.MultiScaleSpectralDiscriminator([512, 128], partial(D.EncodecConvNet, capacity=8), n_channels=1)


def _descript_discriminator():
    from rave_amd import descript_discriminator as DD
    return DD.DescriptDiscriminator(periods=[3], fft_sizes=[256], n_channels=2)


@pytest.mark.parametrize("name,build", [("v2 MPD+MSD", _v2_discriminator), ("encodec spectral", _spectral_discriminator),
                                        ("descript MPD+MRD", _descript_discriminator)])
def test_discriminator_gradient_buckets_hold_views_that_are_only_4_byte_aligned(name, build):
    """The premise of the misaligned tests, pinned: a GradReducer built the way the benchmark builds the discriminator's
    (default arguments) lays the parameters back to back, last parameter first.  Every net ends in a one-channel conv whose
    bias has one element, so the views behind it start off a 16-byte boundary."""
    from rave_amd import ddp
    red = ddp.GradReducer(list(build().parameters()))
    hist = residues(red)
    print(f"{name}: views by storage_offset % 4: {hist}")
    assert sum(hist.values()) == sum(len(b.params) for b in red.buckets) > 0
    assert hist[1] + hist[2] + hist[3] > 0
    # ... and large tensors are among them (a weight gradient, not only one-element biases)
    big = [v for b in red.buckets for v in b.views if v.storage_offset() % 4 and v.numel() >= 256]
    assert big
    red.remove()


def test_generator_gradient_buckets_of_the_data_parallel_tests_are_all_aligned():
    """Why tests/test_ddp_gpu.py and tests/test_ddp_rccl.py cannot see any of this: they reduce the capacity-16 generator only,
    every parameter of which has a multiple of four elements, so EVERY gradient view of theirs sits on a 16-byte boundary (the
    histogram printed below has entries at residue 0 only).  The kernels' behaviour at a misaligned gradient view is tested by
    tests/test_gpu_misaligned_buckets.py instead."""
    from rave_amd import ddp
    from rave_amd import model as M
    m = M.build_v2(capacity=16, latent_size=16)
    gen = list(m.encoder.parameters()) + list(m.decoder.parameters())
    assert not [tuple(p.shape) for p in gen if p.numel() % 4]
    for bucket_mb, who in ((0.25, "test_ddp_gpu.py"), (32.0, "the benchmark's default")):
        red = ddp.GradReducer(gen, bucket_mb=bucket_mb)
        hist = residues(red)
        print(f"capacity-16 generator, bucket_mb={bucket_mb} ({who}): {len(red.buckets)} buckets, views by storage_offset % 4: {hist}")
        assert hist == {0: len(gen), 1: 0, 2: 0, 3: 0}
        red.remove()
