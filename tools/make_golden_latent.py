#!/usr/bin/env python
"""Writes tests/golden/latent_tiny.pt from the UNMODIFIED reference ``RAVE.validation_epoch_end`` (rave/model.py:445-495, with
rave/core.py:180-217 for the receptive field) on the CPU.

    python tools/make_golden_latent.py         # needs the reference tree (oracle/ref_import.py: RAVE_REFERENCE_ROOT)

Recorded data only (tensors, numbers, names):
  * "tiny" / "tiny_causal": the reference v2 at capacity 4, latent_size 8, both under ONE set of weights (the padding mode
    changes no shape).  The state_dict travels as the oracle's seeded parameters ("shapes" + "seed":
    rave_oracle.seeded_state_dict, as tests/golden/v2_wide.pt does) plus every buffer as stored ("buffers", taken after the
    analysis: latent_pca, latent_mean and fidelity are among them).  ``validation_epoch_end`` runs on a synthetic ``out`` list
    of 3 batches of (audio, mean); what it leaves in latent_mean / latent_pca / fidelity / receptive_field and the four
    fidelity_p log values.
  * "wide": a reference model at latent_size 128 fed 3 batches of mean (2, 128, 160), 960 rows (its receptive field is preset:
    only the analysis is recorded, no weights).
  * for each, the same quantities from a float64 restatement in numpy ("f64": mean, SVD of the centred rows, sklearn's sign
    convention on the rows of V) and "ref_err", the reference's own distance from it: max |mean difference|, max |fidelity
    difference|, max over i of 1 - |<ref_i, f64_i>| between the normalised rows (direction_error).
What the reference touches besides the model is stubbed: trainer.state.stage, log (the oracle's Lightning shim keeps a dict),
logger.experiment.add_audio.

The posterior means are synthetic with an imposed covariance spectrum (lambda_i ~ decay^i in a random orthonormal basis) and a
mean of about 0.5 per channel: wide eigenvalue gaps, identifiable components.  decay = 0.6 at 8 channels; 0.95 at 128, where
0.6^127 would leave most of the spectrum below float32 resolution of the largest eigenvalue.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEED = 31
TINY = dict(capacity=4, latent_size=8)
TINY_MEAN = (2, 8, 16)       # per batch; 3 batches = 96 rows
WIDE_MEAN = (2, 128, 160)    # per batch; 3 batches = 960 rows
N_BATCHES = 3
PERCENT = (.8, .9, .95, .99)


def synthetic_out(shape, decay, seed):
    """3 x (audio, mean): mean[b, :, t] = m + Q diag(sqrt(lambda)) g, lambda_i = decay^i, Q orthonormal, m ~ 0.5."""
    b, c, t = shape
    gen = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(c, c, generator=gen, dtype=torch.float64))
    lam = decay ** torch.arange(c, dtype=torch.float64)
    m = 0.5 + 0.1 * torch.randn(c, generator=gen, dtype=torch.float64)
    out = []
    for _ in range(N_BATCHES):
        g = torch.randn(b, t, c, generator=gen, dtype=torch.float64)
        z = (g * lam.sqrt()) @ q.T + m
        audio = torch.randn(b, 1, 64, generator=gen)
        out.append((audio, z.permute(0, 2, 1).contiguous().float()))
    return out


def restate_f64(out):
    """The analysis of rave/model.py:466-481 in float64 (numpy): mean, PCA by SVD of the centred rows with the largest-magnitude
    entry of every row of V made positive, cumulative explained-variance ratio."""
    z = np.concatenate([m.double().numpy().transpose(0, 2, 1).reshape(-1, m.shape[1]) for _, m in out], 0)
    mu = z.mean(0)
    _, s, vt = np.linalg.svd(z - mu, full_matrices=False)
    pick = np.argmax(np.abs(vt), axis=1)
    vt = vt * np.sign(vt[np.arange(vt.shape[0]), pick])[:, None]
    lam = s ** 2 / (z.shape[0] - 1)
    fid = np.cumsum(lam / lam.sum())
    return dict(latent_mean=torch.from_numpy(mu), latent_pca=torch.from_numpy(vt.copy()), fidelity=torch.from_numpy(fid),
                explained_variance=torch.from_numpy(lam))


def direction_error(rows, truth):
    """1 - |<a, b>| per row for the DIRECTIONS a = row / |row|, b = truth / |truth| (float64), computed as |a -+ b|^2 / 2, which
    is the same number without the cancellation.  The rows are normalised first because a unit vector stored in float32 has
    a norm of 1 +- 6e-8: against the raw rows 1 - |<row, truth>| is that norm error (either sign), not a distance."""
    a = rows.double() / rows.double().norm(dim=1, keepdim=True)
    b = truth.double() / truth.double().norm(dim=1, keepdim=True)
    s = torch.sign((a * b).sum(1, keepdim=True))
    return 0.5 * (a - s * b).pow(2).sum(1)


def run_reference(model, out):
    model.trainer = types.SimpleNamespace(state=types.SimpleNamespace(stage=None))
    model.logger = types.SimpleNamespace(experiment=types.SimpleNamespace(add_audio=lambda *a, **k: None))
    model.logged = {}
    with torch.no_grad():
        model.validation_epoch_end(out)
    rec = dict(latent_mean=model.latent_mean.clone(), latent_pca=model.latent_pca.clone(), fidelity=model.fidelity.clone(),
               receptive_field=model.receptive_field.clone(),
               fidelity_p={str(p): float(model.logged[f"fidelity_{p}"]) for p in PERCENT})
    f64 = restate_f64(out)
    rec["f64"] = f64
    rec["ref_err"] = dict(latent_mean=float((rec["latent_mean"].double() - f64["latent_mean"]).abs().max()),
                          fidelity=float((rec["fidelity"].double() - f64["fidelity"]).abs().max()),
                          latent_pca=float(direction_error(rec["latent_pca"], f64["latent_pca"]).max()))
    rec["signs_agree"] = bool((torch.sign(rec["latent_pca"].double()) == torch.sign(f64["latent_pca"])).all())
    rec["mean"] = [m for _, m in out]
    rec["audio"] = [a for a, _ in out]
    return rec


def main() -> None:
    from ref_models import build_reference_rave
    import sklearn
    import rave_oracle as O
    m = build_reference_rave("v2", causal=False, **TINY)
    shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
    sd = O.seeded_state_dict(shapes, SEED)
    assert set(sd) == set(shapes), sorted(set(shapes) - set(sd))
    m.load_state_dict(sd, strict=False)
    out_tiny = synthetic_out(TINY_MEAN, 0.6, SEED + 1)
    golden = dict(config=dict(TINY), seed=SEED, sklearn=sklearn.__version__, shapes=shapes)
    golden["tiny"] = run_reference(m, out_tiny)
    mc = build_reference_rave("v2", causal=True, **TINY)
    mc.load_state_dict(sd, strict=False)
    golden["tiny_causal"] = run_reference(mc, out_tiny)
    for k in ("mean", "audio"):                 # the same `out` as "tiny": stored once
        del golden["tiny_causal"][k]
    wide = build_reference_rave("v2", causal=False, capacity=4, latent_size=128)
    wide.receptive_field[:] = 1                 # only the analysis is recorded for this one
    golden["wide"] = run_reference(wide, synthetic_out(WIDE_MEAN, 0.95, SEED + 2))
    del golden["wide"]["receptive_field"], golden["wide"]["audio"]
    # (the loss modules' STFT windows stay behind, as in the other fixtures: the drop-in distances keep theirs outside the state_dict)
    keep = ("pqmf.", "encoder.", "decoder.", "discriminator.", "latent_pca", "latent_mean", "fidelity", "receptive_field")
    assert all(k.startswith(keep) for k in shapes)
    golden["buffers"] = {k: v.detach().clone() for k, v in m.state_dict().items() if k not in shapes and k.startswith(keep)}
    for tag in ("tiny", "tiny_causal", "wide"):
        r = golden[tag]
        print(tag, "receptive_field", r.get("receptive_field", None), "fidelity_p", r["fidelity_p"], "ref_err", r["ref_err"],
              "signs_agree", r["signs_agree"])
    path = os.path.join(ROOT, "tests", "golden", "latent_tiny.pt")
    torch.save(golden, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
