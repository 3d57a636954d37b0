"""Latent-space analysis on the host (rave_amd/latent.py, the ``latent_analysis`` keyword of rave_amd.model.RAVE) against
tests/golden/latent_tiny.pt: what the reference's own ``validation_epoch_end`` (rave/model.py:445-488, sklearn's PCA) left in
latent_mean / latent_pca / fidelity for a synthetic list of posterior means, and a float64 restatement of the same analysis.

The bar is the reference's: for the mean, the fidelity and the components, the distance from the float64 restatement may not
exceed the reference's own (``ref_err`` in the fixture; at the time of writing 3.7e-8 / 5.0e-8 / 8.7e-13 at 8 channels and
9.3e-8 / 1.4e-7 / 1.1e-9 at 128; the component figure is 1 - |cos| between the normalised rows, latent_cases.distances)."""
import pytest
import torch

import latent_cases as LC


def analyse(rec):
    from rave_amd.latent import LatentAnalysis
    la = LatentAnalysis()
    for _, mean in LC.out_list(rec):
        la.update(mean)
    return la.finish()


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_cpu_path_is_as_close_to_f64_as_the_reference(tag):
    rec = LC.golden()[tag]
    mean, pca, fid = analyse(rec)
    assert mean.dtype == pca.dtype == fid.dtype == torch.float32
    c = rec["mean"][0].shape[1]
    assert mean.shape == (c,) and pca.shape == (c, c) and fid.shape == (c,)
    LC.check_against_fixture(mean, pca, fid, rec)


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_fidelity_percentiles_are_the_reference_integers(tag):
    rec = LC.golden()[tag]
    _, _, fid = analyse(rec)
    assert LC.fidelity_p(fid) == rec["fidelity_p"]


def test_fixture_follows_the_sign_convention():
    """The convention LatentAnalysis.finish restates -- the entry of largest magnitude of every component is positive -- is
    what the reference's PCA produced (sklearn 1.7.2 when the fixture was made), and its float64 restatement agrees."""
    g = LC.golden()
    for tag in ("tiny", "wide"):
        pca = g[tag]["latent_pca"]
        pick = pca.abs().argmax(1, keepdim=True)
        assert bool((pca.gather(1, pick) > 0).all()), tag
        assert g[tag]["signs_agree"] is True


def test_fewer_rows_than_channels_raises():
    from rave_amd.latent import LatentAnalysis
    la = LatentAnalysis()
    la.update(torch.randn(1, 8, 7, generator=torch.Generator().manual_seed(0)))
    with pytest.raises(ValueError):
        la.finish()
    la.update(torch.randn(1, 8, 1, generator=torch.Generator().manual_seed(1)))     # 8 rows for 8 channels: accepted
    assert la.finish() is not None


def test_nothing_fed_is_a_no_op():
    from rave_amd.latent import LatentAnalysis
    la = LatentAnalysis()
    assert la.finish() is None
    la.update(torch.zeros(0, 8, 4))
    assert la.finish() is None


def test_update_is_the_rearranged_rows():
    """(b, t) pairs are the rows: two batches of different (B, T) against the concatenated "b c t -> (b t) c" matrix."""
    from rave_amd.latent import LatentAnalysis
    gen = torch.Generator().manual_seed(5)
    a, b = torch.randn(2, 5, 3, generator=gen) + 0.5, torch.randn(1, 5, 7, generator=gen) - 0.25
    la = LatentAnalysis()
    la.update(a)
    la.update(b)
    z = torch.cat([t.double().permute(0, 2, 1).reshape(-1, 5) for t in (a, b)], 0)
    assert float(la.acc[0]) == z.shape[0]
    torch.testing.assert_close(la.acc[1:6], z.sum(0), rtol=1e-14, atol=0)
    torch.testing.assert_close(la.acc[6:].reshape(5, 5), z.T @ z, rtol=1e-13, atol=1e-14)


def test_state_dict_with_the_keyword_is_todays_plus_three_buffers():
    from rave_amd import model as M
    g = LC.golden()
    cfg = g["config"]
    plain = M.build_v2(**cfg)
    m = M.build_v2(latent_analysis=True, **cfg)
    sd, sd0 = m.state_dict(), plain.state_dict()
    assert set(sd) - set(sd0) == set(LC.ANALYSIS_KEYS) and not set(sd0) - set(sd)
    n = cfg["latent_size"]
    assert torch.equal(sd["latent_pca"], torch.eye(n)) and sd["latent_pca"].dtype == torch.float32
    assert torch.equal(sd["latent_mean"], torch.zeros(n)) and sd["latent_mean"].dtype == torch.float32
    assert torch.equal(sd["fidelity"], torch.zeros(n)) and sd["fidelity"].dtype == torch.float32
    # the reference's state_dict (after its analysis) goes in: nothing unexpected, nothing missing but the receptive field
    ref_sd = LC.fixture_state_dict(g)
    ref_sd.pop("receptive_field")
    res = m.load_state_dict(ref_sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"receptive_field"}, res
    assert torch.equal(m.latent_pca, g["tiny"]["latent_pca"]) and torch.equal(m.fidelity, g["tiny"]["fidelity"])
    for k in LC.ANALYSIS_KEYS:
        assert sd[k].shape == g["buffers"][k].shape and sd[k].dtype == g["buffers"][k].dtype, k


@pytest.mark.parametrize("name", ["build_v1", "build_v2_small", "build_v3", "build_discrete"])
def test_keyword_reaches_every_builder(name):
    from rave_amd import model as M
    kw = dict(capacity=4, latent_size=8)
    if name == "build_discrete":
        kw.update(num_quantizers=2, codebook_size=8, noise_augmentation=2, spectral_capacity=4)
    m = getattr(M, name)(latent_analysis=True, **kw)
    assert m.latent_analysis and tuple(m.latent_pca.shape) == (8, 8)
    assert not set(LC.ANALYSIS_KEYS) & set(getattr(M, name)(**kw).state_dict())


def test_default_build_v2_key_set_is_unchanged():
    """The default stays off: the key set is the one tests/golden/v2_tiny.pt was recorded against, the reference's minus its
    three analysis buffers."""
    import os
    from rave_amd import model as M
    g = LC.golden()
    m = M.build_v2(**g["config"])
    assert m.latent_analysis is False
    ref_keys = set(LC.fixture_state_dict(g))
    assert set(m.state_dict()) == ref_keys - set(LC.ANALYSIS_KEYS)
    old = torch.load(os.path.join(os.path.dirname(LC.GOLDEN), "v2_tiny.pt"), map_location="cpu", weights_only=False)
    assert set(m.state_dict()) == set(old["state_dict"]) | {"receptive_field"}
