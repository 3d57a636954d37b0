"""PQMF with 2, 4, 8 and 32 bands on the HIP kernels of rave_amd/csrc/pqmf_bands.hip (``N_BAND`` of configs/v1.gin rebound):
the four transforms against the unmodified reference's recorded results (tests/golden/pqmf_bands.pt, written by
tools/make_golden_pqmf_bands.py) and the CPU oracle, the drop-in modules, and a shrunk v2 model end to end.

Bounds are the existing ones: TOL_OP (one operator vs CPU fp32) and TOL_E2E (end to end) of tests/test_gpu_parity.py."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import rave_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5
TOL_E2E = 1e-4
BANDS = (2, 4, 8, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(os.path.join(golden_dir, "pqmf_bands.pt"), weights_only=False)


@functools.lru_cache(maxsize=None)
def _bank(m):
    b = O.pqmf_buffers(100, m)
    return b["forward_conv.weight"], b["inverse_conv.weight"], b["hk"]


def _pads(m, causal):
    """(analysis, synthesis) pad pairs: cc.get_padding of the kernels 32 M + 1 and 33, centred or under configs/causal.gin."""
    return ((32 * m, 0), (32, 0)) if causal else ((16 * m, 16 * m), (16, 16))


def _tile_frames(m):
    from rave_amd import _lib as L
    f = L.lib.rh_pqmf_tile_frames(m)        # the kernel's own constant (frames<M>() in pqmf_bands.hip)
    assert f > 0
    return f


# --------------------------------------------------------------------------- the four transforms
@pytest.mark.parametrize("m", BANDS)
def test_fixture_parity(golden, dev, ops, m):
    g = golden[m]
    wf, wi = g["w_fwd"].to(dev), g["w_inv"].to(dev)
    for causal, sfx in ((False, ""), (True, "_causal")):
        pa, ps = _pads(m, causal)
        x = g["x"].to(dev).requires_grad_(True)
        y = ops.pqmf_analysis(x, wf, pa)
        ref = g["y" + sfx]
        assert y.shape == ref.shape
        assert rel_l2(y, ref) < TOL_OP, (causal, rel_l2(y, ref))
        big = ref.abs() > 1e-4              # band / sign indexing: the sign of every non-negligible coefficient agrees
        assert torch.equal(torch.sign(y.detach().cpu())[big], torch.sign(ref)[big])
        (y * g["cot_y"].to(dev)).sum().backward()
        assert rel_l2(x.grad, g["grad_x" + sfx]) < TOL_OP, causal
        yy = ref.to(dev).requires_grad_(True)
        xr = ops.pqmf_synthesis(yy, wi, ps)
        ref = g["x_rec" + sfx]
        assert xr.shape == ref.shape
        assert rel_l2(xr, ref) < TOL_OP, (causal, rel_l2(xr, ref))
        big = ref.abs() > 1e-4
        assert torch.equal(torch.sign(xr.detach().cpu())[big], torch.sign(ref)[big])
        (xr * g["cot_x"].to(dev)).sum().backward()
        assert rel_l2(yy.grad, g["grad_y" + sfx]) < TOL_OP, causal


@pytest.mark.parametrize("m", BANDS)
def test_reverse_half_is_bit_exact(dev, ops, m):
    """A filter that is a pure delta makes analysis a decimating copy: the output equals +-x exactly, with the reverse_half
    pattern (odd band AND even frame -> minus).  One frame more than a workgroup tile, so two workgroups per row."""
    w = torch.zeros(m, 1, 32 * m + 1)
    for k in range(m):
        w[k, 0, 16 * m + k] = 1.0           # band k picks sample M n + k
    n = _tile_frames(m) + 1
    x = torch.randn(2, 1, n * m, generator=torch.Generator().manual_seed(m))
    y = ops.pqmf_analysis(x.to(dev), w.to(dev), (16 * m, 16 * m)).cpu()
    ref = x.reshape(2, n, m).permute(0, 2, 1).clone()
    ref[:, 1::2, ::2] *= -1
    assert torch.equal(y, ref)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("m", BANDS)
def test_vs_oracle_at_the_tile_edges(dev, ops, m, causal):
    """A single frame, three frames, one frame before / at / after the end of a workgroup tile of F frames, and 4096 + M."""
    wf, wi, _ = _bank(m)
    wfd, wid = wf.to(dev), wi.to(dev)
    pa, ps = _pads(m, causal)
    f = _tile_frames(m)
    for rows in (1, 3):
        for t_len in (m, 3 * m, (f - 1) * m, f * m, (f + 1) * m, 4096 + m):
            x = O.synthetic_batch(rows, 1, t_len, seed=t_len + rows)
            y_ref = O.pqmf_analysis(x, wf, causal)
            y = ops.pqmf_analysis(x.to(dev), wfd, pa)
            assert y.shape == y_ref.shape, (rows, t_len)
            assert rel_l2(y, y_ref) < TOL_OP, (rows, t_len, rel_l2(y, y_ref))
            xr_ref = O.pqmf_synthesis(y_ref, wi, causal)
            xr = ops.pqmf_synthesis(y_ref.to(dev), wid, ps)
            assert xr.shape == xr_ref.shape, (rows, t_len)
            assert rel_l2(xr, xr_ref) < TOL_OP, (rows, t_len, rel_l2(xr, xr_ref))


@pytest.mark.parametrize("m", BANDS)
def test_edited_taps_are_honoured(dev, ops, m):
    """Seeded noise of relative size 1e-2 on both weight tensors (the zero taps included): results and input gradients
    follow the oracle's convolution with THOSE weights."""
    wf, wi, _ = _bank(m)
    gen = torch.Generator().manual_seed(100 + m)
    wf = wf + 1e-2 * float(wf.pow(2).mean().sqrt()) * torch.randn(wf.shape, generator=gen)
    wi = wi + 1e-2 * float(wi.pow(2).mean().sqrt()) * torch.randn(wi.shape, generator=gen)
    pa, ps = _pads(m, False)
    x = O.synthetic_batch(2, 1, 96 * m, seed=m).requires_grad_(True)
    y_ref = O.pqmf_analysis(x, wf)
    cy = torch.randn(y_ref.shape, generator=gen)
    (y_ref * cy).sum().backward()
    yy = y_ref.detach().clone().requires_grad_(True)
    xr_ref = O.pqmf_synthesis(yy, wi)
    cx = torch.randn(xr_ref.shape, generator=gen)
    (xr_ref * cx).sum().backward()
    xd = x.detach().to(dev).requires_grad_(True)
    y = ops.pqmf_analysis(xd, wf.to(dev), pa)
    (y * cy.to(dev)).sum().backward()
    yd = y_ref.detach().to(dev).requires_grad_(True)
    xr = ops.pqmf_synthesis(yd, wi.to(dev), ps)
    (xr * cx.to(dev)).sum().backward()
    assert rel_l2(y, y_ref) < TOL_OP and rel_l2(xd.grad, x.grad) < TOL_OP
    assert rel_l2(xr, xr_ref) < TOL_OP and rel_l2(yd.grad, yy.grad) < TOL_OP
    # and the edit is visible at all: the designed bank gives another result
    assert rel_l2(ops.pqmf_analysis(xd.detach(), _bank(m)[0].to(dev), pa), y_ref) > 1e-3


@pytest.mark.parametrize("m", BANDS)
def test_adjointness_reconstruction_and_empty_batch(dev, ops, m):
    """|<A x, c> - <x, A^T c>| < 1e-6 ||A x|| ||c|| for analysis and synthesis (form and constant of
    test_pqmf_full_size_properties) at (2, 1, 4096); synthesis(analysis(x)) against the same composition on the CPU oracle;
    rows == 0."""
    wf, wi, _ = _bank(m)
    wfd, wid = wf.to(dev), wi.to(dev)
    pa, ps = _pads(m, False)
    x = O.synthetic_batch(2, 1, 4096, seed=3 + m)
    gen = torch.Generator().manual_seed(3)
    xa = x.to(dev).requires_grad_(True)
    ya = ops.pqmf_analysis(xa, wfd, pa)
    c = torch.randn(ya.shape, generator=gen).to(dev)
    (ya * c).sum().backward()
    lhs = float((ya.detach().double() * c.double()).sum())
    rhs = float((xa.grad.double() * xa.detach().double()).sum())
    assert abs(lhs - rhs) < 1e-6 * float(ya.detach().double().norm() * c.double().norm())
    yb = torch.randn(ya.shape, generator=gen).to(dev).requires_grad_(True)
    xb = ops.pqmf_synthesis(yb, wid, ps)
    c = torch.randn(xb.shape, generator=gen).to(dev)
    (xb * c).sum().backward()
    lhs = float((xb.detach().double() * c.double()).sum())
    rhs = float((yb.grad.double() * yb.detach().double()).sum())
    assert abs(lhs - rhs) < 1e-6 * float(xb.detach().double().norm() * c.double().norm())
    # run to run: the same bits
    assert torch.equal(ops.pqmf_analysis(xa.detach(), wfd, pa), ya.detach())
    assert torch.equal(ops.pqmf_synthesis(yb.detach(), wid, ps), xb.detach())

    rec_ref = O.pqmf_synthesis(O.pqmf_analysis(x, wf), wi)
    rec = ops.pqmf_synthesis(ya.detach(), wid, ps)
    assert rec.shape == rec_ref.shape and rel_l2(rec, rec_ref) < TOL_OP

    e = ops.pqmf_analysis(torch.zeros(0, 1, 64 * m, device=dev), wfd, pa)
    assert e.shape == (0, m, 64)
    e = ops.pqmf_synthesis(torch.zeros(0, m, 64, device=dev), wid, ps)
    assert e.shape == (0, 1, 64 * m)


# --------------------------------------------------------------------------- the drop-in modules
@pytest.mark.parametrize("m", BANDS)
def test_modules_vs_oracle(dev, m):
    """CachedPQMF and the non-cached PQMF (polyphase and classic) against the oracle's restatement of each form, as
    test_noncached_pqmf_mirror_vs_oracle does for 16 bands."""
    from rave_amd import pqmf as P
    wf, wi, hk = _bank(m)
    g = torch.Generator().manual_seed(9 + m)
    x = torch.randn(3, 1, 96 * m, generator=g)
    y = torch.randn(3, m, 96, generator=g)
    c = P.CachedPQMF(100, m).to(dev)
    assert {k: tuple(v.shape) for k, v in c.state_dict().items()} == {
        "hk": (m, 32 * m), "h": tuple(c.h.shape), "forward_conv.weight": (m, 1, 32 * m + 1), "inverse_conv.weight": (m, m, 33)}
    assert rel_l2(c(x.to(dev)), O.pqmf_analysis(x, wf)) < TOL_OP
    assert rel_l2(c.inverse(y.to(dev)), O.pqmf_synthesis(y, wi)) < TOL_OP
    for polyphase in (True, False):
        p = P.PQMF(attenuation=100, n_band=m, polyphase=polyphase).to(dev)
        assert set(p.state_dict().keys()) == {"hk", "h"} and torch.equal(p.hk.cpu(), hk)
        fa = O.pqmf_polyphase_forward if polyphase else O.pqmf_classic_forward
        fs = O.pqmf_polyphase_inverse if polyphase else O.pqmf_classic_inverse
        assert rel_l2(p(x.to(dev)), fa(x, hk)) < TOL_OP, polyphase
        assert rel_l2(p.inverse(y.to(dev)), fs(y, hk)) < TOL_OP, polyphase


# --------------------------------------------------------------------------- end to end
# The 2048-point scale of the multiband distance reflect-pads its input by 1024 band samples (on the reference as well), so
# a clip needs more than 1024 M samples; the next multiple of the latent rate (128 M) is 1152 M = 9 latent frames, as in
# tests/test_gpu_mel.py.  Capacity 16 / latent 16: the smallest the tiny-model tests use.
KW = dict(capacity=16, latent_size=16)
FRAMES = 9


def _e2e_fixture(m):
    cfg = O.v2_config(n_band=m, **KW)
    sd = O.init_state_dict(cfg, seed=0)
    x = O.synthetic_batch(2, 1, FRAMES * 128 * m, seed=60 + m)
    eps = torch.randn(2, KW["latent_size"], FRAMES, generator=torch.Generator().manual_seed(7))
    return cfg, sd, x, eps


def _oracle_vae_step(cfg, sd, x, eps, dtype):
    def leaf(k, v):
        return v.is_floating_point() and k.startswith(("encoder.", "decoder."))
    sdd = {k: (v.to(dtype).clone().requires_grad_(leaf(k, v)) if v.is_floating_point() else v) for k, v in sd.items()}
    loss_gen, _, parts, out = O.generator_losses(x.to(dtype), sdd, cfg, eps.to(dtype), warmed_up=False)
    loss_gen.backward()
    return sdd, parts, out


@pytest.mark.parametrize("m", [8, 32])
def test_shrunk_v2_forward_and_vae_step_vs_oracle(dev, m):
    """build_v2(n_band=M) against the CPU oracle with cfg.n_band = M: the forward pass at TOL_E2E, the losses of one
    VAE-phase training_step at TOL_E2E, and its parameter gradients against the float64 oracle the way
    test_training_step_golden compares them (the reference's own fp32 error class), plus what the COUNTED LeakyReLU gate
    flips downstream of a tensor account for (tests/gate_flips.py; nothing without a flip)."""
    from gate_flips import OracleGates, chain_flips, flip_allowance_by_param, name_gate_log
    from rave_amd import model as M, ops as R
    cfg, sd, x, eps = _e2e_fixture(m)
    sd32, parts, ref = _oracle_vae_step(cfg, sd, x, eps, torch.float32)
    with OracleGates() as og:
        sd64, _, _ = _oracle_vae_step(cfg, sd, x, eps, torch.float64)

    model = M.build_v2(n_band=m, **KW)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"receptive_field", "encoder.warmed_up"}, res
    for k, v in model.state_dict().items():
        if k.startswith("pqmf."):
            assert torch.equal(v, sd[k]), k
    model = model.to(dev).train()
    xd, ed = x.to(dev), eps.to(dev)
    R.gate_log_begin()
    zp, x_mb = model.encode(xd, return_mb=True)
    z, reg = model.encoder.reparametrize(zp, ed)[:2]
    y_mb = model.decoder(z)
    log = name_gate_log(R.gate_log_end(), model)
    y_raw = model.decode(z)
    assert x_mb.shape == (2, m, FRAMES * 128)
    assert rel_l2(x_mb, ref["x_mb"]) < TOL_OP
    for k, got in (("z_params", zp), ("y_mb", y_mb), ("y_raw", y_raw)):
        assert got.shape == ref[k].shape, k
        assert rel_l2(got, ref[k]) < TOL_E2E, (k, rel_l2(got, ref[k]))

    model.configure_optimizers()
    logged = model.training_step(xd.clone(), 0, eps=ed)
    seen = 0
    for k, v in parts.items():
        if k in logged and torch.is_tensor(logged[k]):
            assert abs(float(logged[k]) - float(v)) <= TOL_E2E * max(1.0, abs(float(v))), (k, float(logged[k]), float(v))
            seen += 1
    assert seen >= 3
    flips, n_gates, _ = chain_flips(log, og.masks[:sum(1 for _, t in log if t is not None)])      # as smoke() pairs them
    allow = flip_allowance_by_param(log, flips)
    named = dict(model.named_parameters())
    checked = 0
    for k, v in sd32.items():
        if not torch.is_tensor(v) or v.grad is None:
            continue
        assert named[k].grad is not None, k
        exact = sd64[k].grad
        ref_err = rel_l2(v.grad, exact)
        err = rel_l2(named[k].grad, exact)
        assert err < max(5.0 * ref_err, 5e-4) + 3.0 * allow.get(k, 0.0), (k, err, ref_err, allow.get(k, 0.0))
        checked += 1
    print(f"n_band {m}: {checked} gradients checked, {sum(flips)} of {n_gates} gates flipped against float64")
    assert checked >= 50


@pytest.mark.parametrize("m", [8, 32])
def test_graphed_step_is_bit_identical_to_eager(dev, m):
    """One recorded GraphedTrainingStep, replayed twice, against two eager steps (the pattern of
    test_graphed_training_step_is_bit_identical_to_eager): the new analysis kernel publishes no range, the encoder's first
    convolution takes it through the miss path, and that still records."""
    from rave_amd import model as M

    def run(graphed):
        torch.manual_seed(0)
        model = M.build_v2(n_band=m, **KW).to(dev).train()
        model.configure_optimizers(capturable=True)
        xs = [O.synthetic_batch(2, 1, FRAMES * 128 * m, seed=70 + m + i).to(dev) for i in range(2)]
        gen = torch.Generator().manual_seed(2)
        es = [torch.randn(2, KW["latent_size"], FRAMES, generator=gen).to(dev) for _ in range(2)]
        step = M.GraphedTrainingStep(model, xs[0], inject_eps=True) if graphed else None
        for i in range(2):
            if graphed:
                step(xs[i], i, eps=es[i])
            else:
                model.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
            model.on_train_batch_end(None, None, i)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in model.named_parameters()}, (step.logged if graphed else model.logged)

    pe, le = run(False)
    pg, lg = run(True)
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    torch.manual_seed(0)
    m0 = M.build_v2(n_band=m, **KW)
    moved = sum(1 for k, v in m0.named_parameters()
                if k.startswith(("encoder.", "decoder.")) and not torch.equal(v.detach(), pe[k].cpu()))
    assert moved > 50                      # the optimizer really ran
    for k in ("fullband_spectral_distance", "multiband_spectral_distance", "regularization"):
        assert torch.equal(le[k].detach(), lg[k].detach()), k
