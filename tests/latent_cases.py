"""What tests/test_latent_host.py and tests/test_gpu_latent.py share (a plain helper module, no fixtures): the fixture
tests/golden/latent_tiny.pt (tools/make_golden_latent.py) and the three distances its ``ref_err`` is stated in."""
import os

import torch

import rave_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_tiny.pt")
ANALYSIS_KEYS = ("latent_pca", "latent_mean", "fidelity")
PERCENT = (.8, .9, .95, .99)

_G = {}


def golden():
    if not _G:
        _G.update(torch.load(GOLDEN, map_location="cpu", weights_only=False))
    return _G


def fixture_state_dict(g):
    """The reference model's state_dict after its validation_epoch_end: the seeded parameters and the stored buffers."""
    sd = O.seeded_state_dict(g["shapes"], g["seed"])
    sd.update(g["buffers"])
    return sd


def out_list(rec, device="cpu"):
    """The ``out`` list the reference was given: [(audio, mean)] (only the means were kept for the wide case)."""
    audio = rec.get("audio") or [None] * len(rec["mean"])
    return [(a if a is None else a.to(device), m.to(device)) for a, m in zip(audio, rec["mean"])]


def distances(latent_mean, latent_pca, fidelity, f64):
    """The three figures of ``ref_err``, for any f32 result against the fixture's float64 restatement."""
    # 1 - |<a, b>| between the normalised rows, as |a -+ b|^2 / 2 (the same number without the cancellation), exactly as the
    # tool computed the reference's: against rows stored in float32 the raw 1 - |<row, truth>| is the norm's rounding error
    a = latent_pca.detach().cpu().double()
    a = a / a.norm(dim=1, keepdim=True)
    b = f64["latent_pca"] / f64["latent_pca"].norm(dim=1, keepdim=True)
    away = 0.5 * (a - torch.sign((a * b).sum(1, keepdim=True)) * b).pow(2).sum(1)
    return dict(latent_mean=float((latent_mean.detach().cpu().double() - f64["latent_mean"]).abs().max()),
                fidelity=float((fidelity.detach().cpu().double() - f64["fidelity"]).abs().max()),
                latent_pca=float(away.max()))


def check_against_fixture(latent_mean, latent_pca, fidelity, rec):
    """At least as close to the float64 restatement as the reference is (its own figures, read from the fixture), the
    reference's signs, and sklearn's convention itself: the entry of largest magnitude of every row is positive."""
    got = distances(latent_mean, latent_pca, fidelity, rec["f64"])
    print("distance from the f64 restatement:", got, "reference:", rec["ref_err"])
    for k, bound in rec["ref_err"].items():
        assert got[k] <= bound, (k, got[k], bound)
    pca = latent_pca.detach().cpu()
    along = (pca.double() * rec["latent_pca"].double()).sum(1)          # +1: same component, same orientation; -1: flipped
    assert bool((along > 0.99).all()), along
    pick = pca.abs().argmax(1, keepdim=True)
    assert bool((pca.gather(1, pick) > 0).all())


def fidelity_p(fidelity):
    """rave/model.py:483-488: np.argmax(var > p) as a float, for the four percentages."""
    return {str(p): float(torch.argmax((fidelity.detach().cpu() > p).to(torch.uint8))) for p in PERCENT}
