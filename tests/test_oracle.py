"""CPU tests that PIN THE ORACLE (oracle/rave_oracle.py):
  * against the committed golden fixtures produced by the unmodified reference
    (oracle/make_golden.py).
"""
import os

import pytest
import torch

import rave_oracle as O
from conftest import rel_l2

TOL = 2e-6  # same ATen ops as the reference; only thread-count / summation-order noise is allowed


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), weights_only=False)


def test_pqmf_design_matches_reference_buffers(golden_dir):
    g = _load(golden_dir, "pqmf.pt")
    b = O.pqmf_buffers(100, 16)
    assert b["h"].shape == (377,)
    assert rel_l2(b["h"], g["h"]) < 1e-6
    assert rel_l2(b["hk"], g["hk"]) < 1e-6
    assert rel_l2(b["forward_conv.weight"], g["w_fwd"]) < 1e-6
    assert rel_l2(b["inverse_conv.weight"], g["w_inv"]) < 1e-6


def test_pqmf_closed_form_hk():
    """hk[k,t] = 2 h[t] cos((2k+1) pi/32 (t-188) + (-1)^k pi/4)."""
    import math
    b = O.pqmf_buffers(100, 16)
    h = b["h"].double()
    k = torch.arange(16, dtype=torch.float64).reshape(-1, 1)
    t = torch.arange(377, dtype=torch.float64) - 188
    hk = 2 * h * torch.cos((2 * k + 1) * math.pi / 32 * t + (-1) ** k * math.pi / 4)
    assert (b["hk"][:, 67:67 + 377].double() - hk).abs().max() < 2e-7
    assert b["hk"][:, :67].abs().max() == 0 and b["hk"][:, 67 + 377:].abs().max() == 0


def test_pqmf_analysis_synthesis_golden(golden_dir):
    g = _load(golden_dir, "pqmf.pt")
    x = g["x"].reshape(-1, 1, g["x"].shape[-1])
    y = O.pqmf_analysis(x, g["w_fwd"])
    assert rel_l2(y, g["y"]) < TOL
    assert rel_l2(O.pqmf_synthesis(g["y"], g["w_inv"]), g["x_rec"]) < TOL
    assert rel_l2(O.pqmf_analysis(x, g["w_fwd"], causal=True), g["y_causal"]) < TOL
    assert rel_l2(O.pqmf_synthesis(g["y_causal"], g["w_inv"], causal=True), g["x_rec_causal"]) < TOL


def test_pqmf_direct_formula(golden_dir):
    """SURVEY.md section 8a a5 closed forms, float64 numpy loops on a small slice."""
    import numpy as np
    g = _load(golden_dir, "pqmf.pt")
    x = g["x"][0, 0].double().numpy()
    wf = g["w_fwd"][:, 0].double().numpy()
    xpad = np.concatenate([np.zeros(256), x, np.zeros(256)])
    for n in (0, 1, 7, 128, 255):
        for k in (0, 1, 6, 15):
            v = float(np.dot(wf[k], xpad[16 * n:16 * n + 513]))
            if k % 2 == 1 and n % 2 == 0:
                v = -v
            assert abs(v - float(g["y"][0, k, n])) < 1e-5
    # synthesis: out[16n+i] = 16 sum_c sum_t Wi[15-i,c,t] u[c,n+t-16], u = s*y
    wi = g["w_inv"].double().numpy()
    y = g["y"][0].double().numpy().copy()
    y[1::2, ::2] *= -1
    upad = np.concatenate([np.zeros((16, 16)), y, np.zeros((16, 16))], axis=1)
    for n in (0, 3, 100, 255):
        for i in (0, 5, 15):
            v = 16.0 * float(np.sum(wi[15 - i] * upad[:, n:n + 33]))
            assert abs(v - float(g["x_rec"][0, 0, 16 * n + i])) < 1e-5


def test_reverse_half_is_a_sign_involution():
    x = torch.randn(2, 16, 10)
    y = O.reverse_half(x)
    assert torch.equal(O.reverse_half(y), x)
    sign = (y / x)
    for k in range(16):
        for n in range(10):
            assert sign[0, k, n] == (-1 if (k % 2 == 1 and n % 2 == 0) else 1)


def test_pqmf_roundtrip_is_near_perfect_reconstruction():
    """Appendix B #4: near-PR only (~1e-3), delay 16 samples for the cached form."""
    b = O.pqmf_buffers(100, 16)
    x = O.synthetic_batch(1, 1, 8192, seed=5)
    y = O.pqmf_analysis(x, b["forward_conv.weight"])
    xr = O.pqmf_synthesis(y, b["inverse_conv.weight"])
    err = rel_l2(xr[..., 1024 + 16:-1024], x[..., 1024:-1024 - 16])
    assert err < 5e-3


@pytest.mark.parametrize("name,causal", [("v2_tiny.pt", False), ("v2_tiny_causal.pt", True)])
def test_forward_products_golden(golden_dir, name, causal):
    g = _load(golden_dir, name)
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"], causal=causal)
    sd = g["state_dict"]
    with torch.no_grad():
        out = O.rave_forward(g["x"], sd, cfg, g["eps"])
        assert rel_l2(out["x_mb"], g["x_mb"]) < TOL
        assert rel_l2(out["z_params"], g["z_params"]) < TOL
        assert rel_l2(out["z"], g["z"]) < TOL
        assert rel_l2(out["y_mb"], g["y_mb"]) < TOL
        assert rel_l2(out["y_raw"], g["y_raw"]) < TOL
        feats = O.combine_discriminators(torch.cat([g["x"], g["y_raw"]], 0), sd, cfg)
        assert len(feats) == 8 and all(len(f) == 5 for f in feats)
        for f, last, mid in zip(feats, g["feat_last"], g["feat_mid"]):
            assert rel_l2(f[-1], last) < 5e-6
            assert rel_l2(f[2], mid) < 5e-6


def _leaves(g, dtype=torch.float32):
    return {k: (v.to(dtype) if v.is_floating_point() else v).clone().requires_grad_(
        v.is_floating_point() and not k.startswith("pqmf.h")) for k, v in g["state_dict"].items()}


@pytest.mark.parametrize("phase", ["vae", "dis", "gen"])
def test_training_step_losses_and_grads_golden(golden_dir, phase):
    """Losses of the oracle step == the reference's (1e-5 class).  Gradients through the
    spectral losses are ill-conditioned (d log(|STFT|+1e-7) up to 1e7): the reference's own fp32
    gradient is ~0.5-1 % away from a float64 evaluation and only reproducible to that level across
    CPUs, so here they are compared with the float64 oracle at the reference's own error class;
    the tight check is test_backward_with_golden_cotangents."""
    g = _load(golden_dir, "v2_tiny.pt")
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"])
    ref = g[phase]

    def run(dtype):
        sd = _leaves(g, dtype)
        x = g["x"].to(dtype).clone().requires_grad_(True)
        loss_gen, loss_dis, parts, _ = O.generator_losses(x, sd, cfg, g["eps"].to(dtype), warmed_up=phase != "vae")
        (loss_dis if phase == "dis" else loss_gen).backward()
        return sd, parts, loss_dis

    sd, parts, loss_dis = run(torch.float32)
    for k, v in ref["losses"].items():
        if k == "loss_dis":
            if phase != "vae":
                assert abs(float(loss_dis) - float(v)) < 1e-4 * max(1.0, abs(float(v)))
            continue
        if k not in parts:   # pred_real / pred_fake / beta_factor: logging only
            continue
        assert abs(float(parts[k]) - float(v)) <= 2e-5 * max(1.0, abs(float(v))), k
    sd64, _, _ = run(torch.float64)
    checked = 0
    for k, gref in ref["grads"].items():
        got = sd[k].grad
        if got is None:
            assert float(gref.abs().max()) == 0.0
            continue
        exact = sd64[k].grad
        assert rel_l2(got, exact) < max(5.0 * rel_l2(gref, exact), 5e-4), k
        checked += 1
    assert checked >= 5


@pytest.mark.parametrize("phase", ["vae", "gen"])
def test_backward_with_golden_cotangents(golden_dir, phase):
    """Injecting the stored dL/dy_raw, dL/dy_mb of the reference's step into the oracle's hot-path
    backward reproduces the reference's parameter gradients (well-conditioned, <= 2e-5)."""
    g = _load(golden_dir, "v2_tiny.pt")
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"])
    sd = _leaves(g)
    x_mb = O.pqmf_encode(g["x"], sd["pqmf.forward_conv.weight"])
    zp = O.encoder_v2(x_mb, sd, cfg)
    if phase == "gen":
        zp = zp.detach()
    z, reg = O.reparametrize(zp, g["eps"])
    y_mb = O.generator_v2(z, sd, cfg)
    y_raw = O.pqmf_decode(y_mb, sd["pqmf.inverse_conv.weight"], 1)
    cots = g[phase]["cotangents"]
    outs, cs = [y_raw, y_mb], [cots["y_raw"], cots["y_mb"]]
    if phase == "vae":
        outs.append(reg); cs.append(torch.ones(()))
    torch.autograd.backward(outs, cs)
    checked = 0
    for k, gref in g[phase]["grads"].items():
        if k.startswith("discriminator."):
            continue
        assert rel_l2(sd[k].grad, gref) < 2e-5, (k, rel_l2(sd[k].grad, gref))
        checked += 1
    assert checked >= 3


def test_v3_generator_side_golden(golden_dir):
    """Snake + AdaIN (identity in training) + causal padding + stereo (configs/v3.gin, causal.gin):
    oracle forward products and every parameter gradient (incl. Snake alphas) vs the reference."""
    g = _load(golden_dir, "v3_gen_tiny.pt")
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"], n_channels=2, causal=True,
                      activation="snake", adain=True)
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and k in g["grads"]) for k, v in g["state_dict"].items()}
    x_mb = O.pqmf_encode(g["x"], sd["pqmf.forward_conv.weight"], True)
    zp = O.encoder_v2(x_mb, sd, cfg)
    z, _ = O.reparametrize(zp, g["eps"])
    y_mb = O.generator_v2(z, sd, cfg)
    y_raw = O.pqmf_decode(y_mb, sd["pqmf.inverse_conv.weight"], 2, True)
    for a, b in ((x_mb, "x_mb"), (zp, "z_params"), (z, "z"), (y_mb, "y_mb"), (y_raw, "y_raw")):
        assert a.shape == g[b].shape and rel_l2(a, g[b]) < TOL, b
    torch.autograd.backward([y_raw, y_mb], [g["cot_raw"], g["cot_mb"]])
    assert len(g["grads"]) > 100
    for k, gref in g["grads"].items():
        assert rel_l2(sd[k].grad, gref) < 2e-5, k


def test_v3_validation_step_adain_eval_golden(golden_dir):
    """RAVE.validation_step under model.eval() (rave/model.py:426-443) with every branch of AdaptiveInstanceNormalization's
    eval forward (rave/blocks.py:898-926): identity on default buffers, running target statistics (learn_y, two batch sizes),
    source statistics + transfer (learn_x), transfer only -- the oracle's adain_forward / validation_step vs the reference."""
    g = _load(golden_dir, "v3_val_tiny.pt")
    c = g["config"]
    cfg = O.v3_config(capacity=c["capacity"], latent_size=c["latent_size"], eval_mode=True)
    sd = {k: v.clone() for k, v in g["state_dict"].items()}
    for call in g["calls"]:
        for name in g["adain_names"]:
            sd[name + ".learn_y"].fill_(call["learn_y"])
            sd[name + ".learn_x"].fill_(call["learn_x"])
        x = g["xs"][call["x_index"]]
        with torch.no_grad():
            audio, mean, dist = O.validation_step(x, sd, cfg, call["eps"])
        assert audio.shape == call["audio"].shape and rel_l2(audio, call["audio"]) < TOL
        assert rel_l2(mean, call["mean"]) < TOL
        assert abs(float(dist) - float(call["distance"])) < 1e-4 * abs(float(call["distance"]))
        for name, bufs in zip(g["adain_names"], call["buffers_after"]):
            for k, v in bufs.items():
                assert rel_l2(sd[f"{name}.{k}"], v) < TOL or float((sd[f"{name}.{k}"] - v).abs().max()) == 0.0, (name, k)
    last = g["calls"][-1]["buffers_after"][0]
    assert float(last["num_update_y"]) == 2 and float(last["num_update_x"]) == 1        # the script really walked the branches
    assert float((last["std_x"][:2] - 1).abs().max()) > 1e-3


def test_v2_small_noise_generator_golden(golden_dir):
    """configs/v2_small.gin: NoiseGeneratorV2 branch of GeneratorV2 (rave/blocks.py:243-292,696-711)."""
    g = _load(golden_dir, "v2_small_tiny.pt")
    c = g["config"]
    cfg = O.v2_small_config(capacity=c["capacity"], latent_size=c["latent_size"])
    sd = {k: v.clone().requires_grad_(k in g["grads"]) for k, v in g["state_dict"].items()}
    zp = O.encoder_v2(O.pqmf_encode(g["x"], sd["pqmf.forward_conv.weight"]), sd, cfg)
    assert rel_l2(zp, g["z_params"]) < TOL
    z, _ = O.reparametrize(zp, g["eps"])
    y_mb = O.generator_v2(z, sd, cfg, noise=g["noise"])
    assert rel_l2(y_mb, g["y_mb"]) < TOL
    assert rel_l2(O.pqmf_decode(y_mb, sd["pqmf.inverse_conv.weight"], 1), g["y_raw"]) < TOL
    torch.autograd.backward([y_mb], [g["cot_mb"]])
    for k, gref in g["grads"].items():
        assert rel_l2(sd[k].grad, gref) < 2e-5, k


def test_init_state_dict_layout_matches_golden(golden_dir):
    g = _load(golden_dir, "v2_tiny.pt")
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"])
    mine = O.init_state_dict(cfg)
    ref = {k: v for k, v in g["state_dict"].items() if k != "encoder.warmed_up"}
    assert set(mine) == set(ref)
    for k in ref:
        assert tuple(mine[k].shape) == tuple(ref[k].shape), k


# ---- comparison with the unmodified reference's own classes (their outputs: tests/golden/reference_checks.pt) -----------
@pytest.mark.parametrize("causal", [False, True])
def test_oracle_equals_reference_modules(golden_dir, causal):
    ref = _load(golden_dir, "reference_checks.pt")
    base, g = ref["modules"], ref["modules_causal" if causal else "modules"]
    sd = O.seeded_state_dict(base["shapes"], base["seed"])
    sd.update(base["weight_g"])
    sd.update({"pqmf." + k: v for k, v in O.pqmf_buffers(100, 16).items()})
    out = lambda v: _sub(v, base["out_step"], base["out_keep"])
    cfg = O.v2_config(capacity=10, latent_size=12, causal=causal)
    x = base["x"]
    with torch.no_grad():
        out_mb = O.pqmf_encode(x, sd["pqmf.forward_conv.weight"], causal)
        assert rel_l2(out(out_mb), g["x_mb"]) < TOL
        zp = O.encoder_v2(out_mb, sd, cfg)
        assert rel_l2(zp, g["z_params"]) < TOL
        y_mb = O.generator_v2(g["z"], sd, cfg)
        assert rel_l2(out(y_mb), g["y_mb"]) < TOL
        yr = O.pqmf_decode(y_mb, sd["pqmf.inverse_conv.weight"], 1, causal)
        assert rel_l2(out(yr), g["y_raw"]) < TOL
        fo = O.combine_discriminators(torch.cat([x, yr], 0), sd, cfg)
        assert [[tuple(f.shape) for f in net] for net in fo] == g["feature_shapes"]
        for a, b in zip(g["features"], fo):
            for u, v in zip(a, b):
                assert rel_l2(_sub(v, base["feature_step"], base["feature_keep"]), u) < 5e-6
        assert abs(float(O.audio_distance_v1(x, yr, cfg)) - float(g["spectral_distance"])) < 1e-4


def test_reference_polyphase_and_classic_forms_agree_with_cached(golden_dir):
    """CachedPQMF.forward == polyphase_forward == classic_forward."""
    g = _load(golden_dir, "reference_checks.pt")["pqmf_forms"]
    b = O.pqmf_buffers(100, 16)
    y = O.pqmf_analysis(g["x"], b["forward_conv.weight"])
    assert rel_l2(g["polyphase"], y) < 2e-6 and rel_l2(g["classic"], y) < 2e-6


# --------------------------------------------------------------------------- general-Conv2d discriminators
def _oracle_disc_check(g, feats_of, sd):
    x = g["x"].clone().requires_grad_(True)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    feats = feats_of(x, params)
    assert [len(n) for n in feats] == [len(n) for n in g["features"]]
    for net, gnet in zip(feats, g["features"]):
        for f, gf in zip(net, gnet):
            assert f.shape == gf.shape
            assert rel_l2(f, gf) < 1e-5
    loss = sum(f.pow(2).mean() for net in feats for f in net)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    assert rel_l2(x.grad, g["dx"]) < 1e-4
    for k, ref in g["grads"].items():
        got = params["d." + k].grad.reshape(-1)
        got = got if got.numel() <= 200_000 else got[::g["grad_step"]]
        assert rel_l2(got, ref) < 1e-4, k


def test_oracle_encodec_discriminator_matches_reference_golden(golden_dir):
    g = torch.load(os.path.join(golden_dir, "disc2d_tiny.pt"), weights_only=False)["encodec"]
    sd = {"d." + k: v for k, v in g["state_dict"].items()}
    # the seed reproduces the stored weights (what the descript fixture relies on)
    again = O.seeded_state_dict(g["shapes"], g["seed"])
    assert all(torch.equal(again[k], g["state_dict"][k]) for k in again)
    _oracle_disc_check(g, lambda x, p: O.multiscale_spectral_discriminator(x, p, "d", g["config"]["scales"]), sd)


def test_oracle_descript_discriminator_matches_reference_golden(golden_dir):
    g = torch.load(os.path.join(golden_dir, "disc2d_tiny.pt"), weights_only=False)["descript"]
    sd = {"d." + k: v for k, v in O.seeded_state_dict(g["shapes"], g["seed"]).items()}
    c = g["config"]
    _oracle_disc_check(g, lambda x, p: O.descript_discriminator(x, p, "d", c["periods"], c["fft_sizes"]), sd)


# --------------------------------------------------------------------------- RVQ
@pytest.mark.parametrize("tag", ["small", "wide"])
def test_oracle_rvq_matches_reference_golden(golden_dir, tag):
    g = torch.load(os.path.join(golden_dir, "rvq_tiny.pt"), weights_only=False)[tag]
    c = g["config"]
    sd = {"r." + k: v for k, v in g["sd0"].items()}
    z = g["z"].clone().requires_grad_(True)
    q, loss, ind, new = O.rvq_forward(z, sd, "r", c["num_quantizers"], training=True)
    assert torch.equal(ind, g["ind"])                       # index work: exact
    assert rel_l2(q, g["q"]) < 1e-6 and abs(float(loss.detach()) - float(g["loss"])) < 1e-6 * abs(float(g["loss"]))
    ((q * g["cot"]).sum() + 3.0 * loss).backward()
    assert rel_l2(z.grad, g["dz"]) < 1e-6
    for k, v in new.items():
        assert rel_l2(v, g["sd1"][k[2:]]) < 1e-6, k
    sd1 = {"r." + k: v for k, v in g["sd1"].items()}
    qe, le, ie, _ = O.rvq_forward(g["z"], sd1, "r", c["num_quantizers"], training=False)
    assert torch.equal(ie, g["ind_eval"]) and rel_l2(qe, g["q_eval"]) < 1e-6 and float(le) == 0.0


def test_oracle_noncached_pqmf_variants_match_reference(golden_dir):
    """PQMF (polyphase / classic, rave/pqmf.py:92-242) restated; pinned to the reference classes' outputs and
    to the documented relation with the cached bank: same analysis, synthesis advanced by one 16-sample frame."""
    b = O.pqmf_buffers(100, 16)
    hk = b["hk"]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 4096, generator=g)
    y = torch.randn(2, 16, 256, generator=g)
    yc = O.pqmf_analysis(x, b["forward_conv.weight"])
    for f in (O.pqmf_polyphase_forward, O.pqmf_classic_forward):
        assert rel_l2(f(x, hk), yc) < 2e-6
    xc = O.pqmf_synthesis(y, b["inverse_conv.weight"])
    for f in (O.pqmf_polyphase_inverse, O.pqmf_classic_inverse):
        out = f(y, hk)
        assert out.shape == xc.shape
        assert rel_l2(out[..., :-16], xc[..., 16:]) < 1e-5
    ref = _load(golden_dir, "reference_checks.pt")["pqmf_noncached"]
    for form, fa, fs in (("polyphase", O.pqmf_polyphase_forward, O.pqmf_polyphase_inverse),
                         ("classic", O.pqmf_classic_forward, O.pqmf_classic_inverse)):
        assert rel_l2(fa(ref["x"], hk), ref[form]["forward"]) < TOL and rel_l2(fs(ref["y"], hk), ref[form]["inverse"]) < TOL


def _sub(g, step, keep):
    g = g.detach().reshape(-1)
    return g if g.numel() <= keep else g[::step]


def test_oracle_reproduces_the_full_width_reference_golden(golden_dir):
    """v2_wide.pt: the reference's own modules at CAPACITY 96 (oracle/make_golden.py:golden_v2_wide) -- outputs and
    parameter gradients under stored cotangents.  Pins the oracle at the benchmarked width."""
    g = _load(golden_dir, "v2_wide.pt")
    cfg = O.v2_config(capacity=g["config"]["capacity"], latent_size=g["config"]["latent_size"])
    sd = O.seeded_state_dict(g["shapes"], g["seed"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    full = dict(leaves)
    full.update({"pqmf." + k: v for k, v in O.pqmf_buffers(100, 16).items()})
    out = O.rave_forward(g["x"], full, cfg, g["eps"])
    for k in ("x_mb", "z_params", "y_mb", "y_raw"):
        assert rel_l2(out[k], g[k]) < TOL, k
    torch.autograd.backward([out["y_raw"], out["y_mb"], out["reg"]], [g["cot_y_raw"], g["cot_y_mb"], torch.ones(())])
    assert len(g["grads"]) == 112
    for k, gref in g["grads"].items():
        got = _sub(leaves[k].grad, g["grad_step"], g["grad_keep"])
        assert rel_l2(got, gref) < 1e-5, (k, rel_l2(got, gref))


def test_stft_loss_algorithm_restatement_vs_torch_stft():
    """oracle/stft_loss_algorithm.py (the algebra of stft_loss.hip: packed frame pairs, Stockham passes with the kernel's
    index arithmetic, Hermitian gradient operand, swap-FFT-swap inverse, overlap-add, margin folds) against torch.stft +
    autograd in f64, the reference's formulation (rave/core.py:269-344)."""
    import numpy as np
    import stft_loss_algorithm as A
    rng = np.random.default_rng(0)
    for n in (128, 256, 512, 1024, 2048):                    # the Stockham passes are the DFT
        z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        assert np.abs(A.stockham_fft(z) - np.fft.fft(z)).max() < 1e-10
    eps = 1e-7
    for n, t, rows, fft in ((128, 1000, 3, A.stockham_fft), (256, 777, 2, np.fft.fft), (512, 4100, 2, np.fft.fft)):
        win = torch.hann_window(n, dtype=torch.float64)
        win = win / win.pow(2).sum().sqrt()
        x = torch.randn(rows, t, dtype=torch.float64, requires_grad=True)
        y = torch.randn(rows, t, dtype=torch.float64, requires_grad=True)
        sx = torch.stft(x, n, n // 4, n, win, center=True, pad_mode="reflect", return_complex=True).abs()
        sy = torch.stft(y, n, n // 4, n, win, center=True, pad_mode="reflect", return_complex=True).abs()
        d = ((sx - sy) ** 2).mean() / (sx ** 2).mean() + (torch.log(sx + eps) - torch.log(sy + eps)).abs().mean()
        d.backward()
        dist, dx, dy = A.distance_and_gradients(x.detach().numpy(), y.detach().numpy(), win.numpy(), eps, fft)
        assert abs(dist - float(d)) <= 1e-12 * abs(float(d))
        assert np.abs(dx - x.grad.numpy()).max() <= 1e-10 * np.abs(x.grad.numpy()).max()
        assert np.abs(dy - y.grad.numpy()).max() <= 1e-10 * np.abs(y.grad.numpy()).max()


@pytest.mark.parametrize("power,normalized,norms", [(1, True, ("L1", "L2")), (2, False, "L2"), (None, True, "L1")])
def test_spectral_and_encodec_distances_equal_the_reference_classes(golden_dir, power, normalized, norms):
    """rave/core.py:415-490 (the rest of SURVEY section 8f #1): rave_amd.losses.SpectralDistance / WaveformDistance /
    EncodecAudioDistance against the reference's own classes (on the torchaudio shim), values and gradients."""
    from functools import partial
    from rave_amd import losses
    ref = _load(golden_dir, "reference_checks.pt")["distances"]
    x, y = ref["x"], ref["y"]
    case = ref["cases"][(power, normalized, norms)]
    kw = dict(sampling_rate=44100, norm=norms, power=power, normalized=normalized)
    for n_fft in (256, 1024):
        b = losses.SpectralDistance(n_fft, **kw)
        yb = y.clone().requires_grad_(True)
        da, db = case[n_fft]["distance"], b(x, yb)
        assert abs(float(da) - float(db)) <= 1e-5 * abs(float(da))
        db.backward()
        assert rel_l2(_sub(yb.grad, ref["out_step"], ref["out_keep"]), case[n_fft]["grad_y"]) < 1e-5
    eb = losses.EncodecAudioDistance([256, 512], partial(losses.SpectralDistance, **kw))
    ra, rb = case["encodec"], eb(x, y)
    assert set(ra) == set(rb) == {"waveform_distance", "spectral_distance"}
    for k in ra:
        assert abs(float(ra[k]) - float(rb[k])) <= 1e-5 * abs(float(ra[k])), k
