"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/*.pt from the UNMODIFIED reference
(/root/reference, imported through oracle/ref_import.py) in the build container.

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py

The reference holds no golden vectors of its own for this path (shape-only
tests); these fixtures are outputs of the reference's own modules on seeded inputs and pin both
the oracle restatement (tests/test_oracle.py, CPU) and the HIP path (tests/test_gpu_parity.py).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from ref_models import attach_optimizers, build_reference_discrete, build_reference_rave  # noqa: E402
import rave_oracle as O  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
torch.set_num_threads(8)


def t(x):
    return x.detach().clone().contiguous()


def golden_pqmf():
    torch.manual_seed(0)
    m = build_reference_rave("v2", capacity=4, latent_size=8)
    pq = m.pqmf
    x = O.synthetic_batch(3, 1, 4096, seed=7)
    with torch.no_grad():
        y = pq(x.reshape(-1, 1, x.shape[-1]))
        xr = pq.inverse(y)
    # gradients of both directions w.r.t. their inputs under a fixed cotangent
    g = torch.Generator().manual_seed(11)
    cy = torch.randn(y.shape, generator=g)
    cx = torch.randn(xr.shape, generator=g)
    xa = x.reshape(-1, 1, x.shape[-1]).clone().requires_grad_(True)
    (pq(xa) * cy).sum().backward()
    ya = y.clone().requires_grad_(True)
    (pq.inverse(ya) * cx).sum().backward()
    out = dict(h=t(pq.h), hk=t(pq.hk), w_fwd=t(pq.forward_conv.weight), w_inv=t(pq.inverse_conv.weight),
               x=t(x), y=t(y), x_rec=t(xr), cot_y=cy, cot_x=cx, grad_x=t(xa.grad), grad_y=t(ya.grad))
    # causal overlay (configs/causal.gin)
    mc = build_reference_rave("v2", capacity=4, latent_size=8, causal=True)
    with torch.no_grad():
        yc = mc.pqmf(x.reshape(-1, 1, x.shape[-1]))
        xc = mc.pqmf.inverse(yc)
    out.update(y_causal=t(yc), x_rec_causal=t(xc))
    build_reference_rave("v2", capacity=4, latent_size=8, causal=False)  # reset gin binding
    torch.save(out, os.path.join(OUT, "pqmf.pt"))
    print("pqmf.pt", {k: tuple(v.shape) for k, v in out.items()})


SELECT = [
    "encoder.encoder.net.0.weight_v", "encoder.encoder.net.0.weight_g",
    "encoder.encoder.net.1.aligned.branches.0.net.1.weight_v",
    "encoder.encoder.net.1.aligned.branches.0.net.3.weight_g",
    "encoder.encoder.net.5.weight_v",
    "decoder.net.0.weight_v", "decoder.net.2.weight_v", "decoder.net.2.weight_g",
    "decoder.net.3.aligned.branches.0.net.1.weight_v", "decoder.net.21.weight_v",
    "discriminator.discriminators.0.layers.0.net.0.weight_v",
    "discriminator.discriminators.0.layers.0.net.0.bias",
    "discriminator.discriminators.0.layers.4.net.4.weight_v",
    "discriminator.discriminators.0.layers.2.net.8.weight",
    "discriminator.discriminators.1.layers.0.net.0.weight_v",
    "discriminator.discriminators.1.layers.2.net.6.weight_g",
    "discriminator.discriminators.1.layers.1.net.8.bias",
]


def grads_of(model):
    named = dict(model.named_parameters())
    return {k: t(named[k].grad) for k in SELECT if named[k].grad is not None}


def oracle_cotangents(sd, x, eps, cfg, phase, ref_grads):
    """dL/dy_raw, dL/dy_mb, dL/dz_params of the step, evaluated by the oracle IN THIS CONTAINER.
    The spectral-loss backward is ill-conditioned (d log(|STFT|+1e-7) reaches 1e7), so these
    cotangents are only reproducible to ~1 % across machines; storing them lets the parity
    tests inject exactly the values the golden parameter gradients were produced with.  The
    oracle's parameter gradients are asserted equal to the reference's first."""
    leaves = {k: v.clone().requires_grad_(v.is_floating_point() and not k.startswith("pqmf.h"))
              for k, v in sd.items()}
    xx = x.clone().requires_grad_(True)
    loss_gen, loss_dis, _, out = O.generator_losses(xx, leaves, cfg, eps, warmed_up=phase != "vae")
    for k in ("y_raw", "y_mb", "z_params"):
        if out[k].requires_grad:
            out[k].retain_grad()
    (loss_dis if phase == "dis" else loss_gen).backward()
    for k, gref in ref_grads.items():
        got = leaves[k].grad
        err = float((got - gref).norm() / gref.norm())
        assert err < 1e-5, (phase, k, err)
    return {k: t(out[k].grad) for k in ("y_raw", "y_mb", "z_params") if out[k].grad is not None}


def golden_v2_tiny(causal=False, name="v2_tiny.pt"):
    cap, lat, n_signal, batch = 6, 8, 32768, 2
    torch.manual_seed(0)
    m = build_reference_rave("v2", capacity=cap, latent_size=lat, causal=causal)
    m.train()
    attach_optimizers(m)
    sd = {k: t(v) for k, v in m.state_dict().items()
          if k.startswith(("pqmf.", "encoder.", "decoder.", "discriminator."))}
    x = O.synthetic_batch(batch, 1, n_signal, seed=3)
    out = dict(config=dict(capacity=cap, latent_size=lat, causal=causal, n_signal=n_signal, batch=batch),
               state_dict=sd, x=t(x))
    # forward products with injected noise (first RNG draw of the step is randn_like(mean))
    with torch.no_grad():
        zp, x_mb = m.encode(x, return_mb=True)
        torch.manual_seed(1234)
        z, reg = m.encoder.reparametrize(zp)[:2]
        torch.manual_seed(1234)
        eps = torch.randn(z.shape)
        y_mb = m.decoder(z)
        y_raw = m.decode(z)
        feats = m.discriminator(torch.cat([x, y_raw], 0))
    out.update(eps=eps, x_mb=t(x_mb), z_params=t(zp), z=t(z), reg=t(reg), y_mb=t(y_mb), y_raw=t(y_raw),
               feat_last=[t(f[-1]) for f in feats], feat_mid=[t(f[2]) for f in feats])
    # VAE-phase step (warmed_up False): rave/model.py:288-413 run by the reference itself
    m.warmed_up = False
    torch.manual_seed(1234)
    m.training_step(x.clone(), 0)
    out["vae"] = dict(losses={k: t(v) for k, v in m.logged.items() if torch.is_tensor(v)}, grads=grads_of(m))
    ocfg = O.v2_config(capacity=cap, latent_size=lat, causal=causal)
    out["vae"]["cotangents"] = oracle_cotangents(sd, x, eps, ocfg, "vae", out["vae"]["grads"])
    # GAN phase from the SAME initial weights
    m.load_state_dict({**m.state_dict(), **sd})
    attach_optimizers(m)
    m.zero_grad(set_to_none=True)
    m.warmed_up = True
    torch.manual_seed(1234)
    m.training_step(x.clone(), 0)   # discriminator step (0 % 4 == 0)
    out["dis"] = dict(losses={k: t(v) for k, v in m.logged.items() if torch.is_tensor(v)}, grads=grads_of(m))
    m.load_state_dict({**m.state_dict(), **sd})
    attach_optimizers(m)
    m.zero_grad(set_to_none=True)
    m.warmed_up = True
    torch.manual_seed(1234)
    m.training_step(x.clone(), 1)   # generator step
    out["gen"] = dict(losses={k: t(v) for k, v in m.logged.items() if torch.is_tensor(v)}, grads=grads_of(m))
    out["gen"]["cotangents"] = oracle_cotangents(sd, x, eps, ocfg, "gen", out["gen"]["grads"])
    torch.save(out, os.path.join(OUT, name))
    nbytes = os.path.getsize(os.path.join(OUT, name))
    print(name, nbytes, "bytes;", {k: float(v) for k, v in out["vae"]["losses"].items()})
    if causal:
        build_reference_rave("v2", capacity=cap, latent_size=lat, causal=False)


def golden_v3_gen_tiny(name="v3_gen_tiny.pt"):
    """Generator side of configs/v3.gin (Snake activations + AdaIN, which is the identity in training
    mode) with causal padding and stereo input (BASELINE configs[4] geometry, shrunk): forward
    products and the parameter gradients under fixed random cotangents at y_raw / y_mb (well
    conditioned), produced by the reference modules."""
    cap, lat, n_signal, batch = 6, 8, 8192, 2
    torch.manual_seed(0)
    m = build_reference_rave("v3", n_channels=2, capacity=cap, latent_size=lat, causal=True)
    m.train()
    with torch.no_grad():   # make the Snake alphas non-trivial
        for n_, p_ in m.named_parameters():
            if n_.endswith("alpha"):
                p_.copy_(0.5 + torch.rand_like(p_))
    sd = {k: t(v) for k, v in m.state_dict().items() if k.startswith(("pqmf.", "encoder.", "decoder."))}
    x = O.synthetic_batch(batch, 2, n_signal, seed=5)
    gen = torch.Generator().manual_seed(77)
    zp, x_mb = m.encode(x, return_mb=True)
    eps = torch.randn(zp.shape[0], lat, zp.shape[-1], generator=gen)
    mean, scale = zp.chunk(2, 1)
    std = torch.nn.functional.softplus(scale) + 1e-4
    z = eps * std + mean
    y_mb = m.decoder(z)
    y_raw = m.decode(z)
    c_raw = torch.randn(y_raw.shape, generator=gen)
    c_mb = torch.randn(y_mb.shape, generator=gen)
    m.zero_grad(set_to_none=True)
    torch.autograd.backward([y_raw, y_mb], [c_raw, c_mb])
    grads = {k: t(p.grad) for k, p in m.named_parameters()
             if p.grad is not None and k.startswith(("encoder.", "decoder."))}
    out = dict(config=dict(capacity=cap, latent_size=lat, n_channels=2, causal=True, n_signal=n_signal, batch=batch),
               state_dict=sd, x=t(x), eps=eps, x_mb=t(x_mb), z_params=t(zp), z=t(z), y_mb=t(y_mb), y_raw=t(y_raw),
               cot_raw=c_raw, cot_mb=c_mb, grads=grads)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", len(grads), "gradients")
    build_reference_rave("v2", capacity=4, latent_size=4, causal=False)   # reset the causal binding


def golden_v3_validation_tiny(name="v3_val_tiny.pt"):
    """RAVE.validation_step (rave/model.py:426-443) of the v3 configuration (Snake + AdaIN, causal, stereo) under
    ``model.eval()``, where AdaptiveInstanceNormalization leaves its training-mode identity (rave/blocks.py:898-926): five
    calls walk every branch -- default buffers (identity), two calls with ``learn_y`` set (running target statistics,
    another batch size), one with ``learn_x`` set (source statistics + transfer), one with both cleared (transfer only).
    Stored per call: the returned cat([x, y], -1), the latent mean, the validation distance; and the buffers left behind."""
    cap, lat, n_signal = 6, 8, 8192
    torch.manual_seed(0)
    m = build_reference_rave("v3", n_channels=2, capacity=cap, latent_size=lat, causal=True)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.endswith("alpha"):
                p_.copy_(0.5 + torch.rand_like(p_))
    m.eval()
    sd = {k: t(v) for k, v in m.state_dict().items() if k.startswith(("pqmf.", "encoder.", "decoder."))}
    from rave import blocks
    adains = [mod for mod in m.modules() if isinstance(mod, blocks.AdaptiveInstanceNormalization)]
    assert len(adains) == 22
    xs = [O.synthetic_batch(2, 2, n_signal, seed=5), O.synthetic_batch(3, 2, n_signal, seed=6),
          O.synthetic_batch(2, 2, n_signal, seed=8)]
    script = [(0, 0, 0), (1, 1, 0), (2, 1, 0), (0, 0, 1), (0, 0, 0)]        # (which x, learn_y, learn_x)
    calls = []
    for n, (xi, ly, lx) in enumerate(script):
        for a in adains:
            a.learn_y.fill_(ly)
            a.learn_x.fill_(lx)
        x = xs[xi]
        seed = 100 + n
        t_lat = n_signal // 16 // 128                     # 16 bands, ratios 4 * 4 * 4 * 2
        torch.manual_seed(seed)
        eps = torch.randn(x.shape[0], lat, t_lat)         # the draw reparametrize makes inside validation_step (its first
        torch.manual_seed(seed)                           # and only consumer of the generator): randn_like(mean)
        with torch.no_grad():
            audio, mean = m.validation_step(x, 0)
            y = audio[..., x.shape[-1]:]
            assert mean.shape == eps.shape
        buffers = [{k_: t(getattr(a, k_)) for k_ in ("mean_x", "std_x", "num_update_x", "mean_y", "std_y", "num_update_y")}
                   for a in adains]
        with torch.no_grad():
            dist = sum(m.audio_distance(x, y).values())
        calls.append(dict(x_index=xi, learn_y=ly, learn_x=lx, eps=eps, audio=t(audio), mean=t(mean), distance=t(dist),
                          buffers_after=buffers))
    names = [n_ for n_, mod in m.named_modules() if isinstance(mod, blocks.AdaptiveInstanceNormalization)]
    out = dict(config=dict(capacity=cap, latent_size=lat, n_channels=2, causal=True, n_signal=n_signal),
               state_dict=sd, xs=[t(x) for x in xs], calls=calls, adain_names=names)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", [float(c["distance"]) for c in calls])
    build_reference_rave("v2", capacity=4, latent_size=4, causal=False)   # reset the causal binding


def golden_v2_small_tiny(name="v2_small_tiny.pt"):
    """configs/v2_small.gin (BASELINE configs[0] family): NoiseGeneratorV2 on the decoder.  Forward
    products of the reference with the uniform noise draw captured (first RNG draw of decoder.forward),
    plus parameter gradients under fixed cotangents."""
    cap, lat, n_signal, batch = 6, 8, 8192, 2
    torch.manual_seed(0)
    m = build_reference_rave("v2_small", capacity=cap, latent_size=lat)
    m.train()
    sd = {k: t(v) for k, v in m.state_dict().items() if k.startswith(("pqmf.", "encoder.", "decoder."))}
    x = O.synthetic_batch(batch, 1, n_signal, seed=8)
    gen = torch.Generator().manual_seed(99)
    zp, x_mb = m.encode(x, return_mb=True)
    eps = torch.randn(zp.shape[0], lat, zp.shape[-1], generator=gen)
    mean, scale = zp.chunk(2, 1)
    z = eps * (torch.nn.functional.softplus(scale) + 1e-4) + mean
    torch.manual_seed(4321)
    y_mb = m.decoder(z)
    # the draw: torch.rand_like(ir) with ir of shape (B, L/8, n_band, 8)
    l_amp = y_mb.shape[-1] // 8
    torch.manual_seed(4321)
    noise = torch.rand(batch, l_amp, 16, 8) * 2 - 1
    cfg = O.v2_small_config(capacity=cap, latent_size=lat)
    chk = O.generator_v2(z.detach(), sd, cfg, noise=noise)
    assert float((chk - y_mb).abs().max()) == 0.0, "captured noise does not reproduce the reference output"
    y_raw = m.pqmf.inverse(y_mb)
    c_mb = torch.randn(y_mb.shape, generator=gen)
    m.zero_grad(set_to_none=True)
    torch.autograd.backward([y_mb], [c_mb])
    grads = {k: t(p.grad) for k, p in m.named_parameters()
             if p.grad is not None and k.startswith(("encoder.", "decoder."))}
    out = dict(config=dict(capacity=cap, latent_size=lat, n_signal=n_signal, batch=batch), state_dict=sd, x=t(x),
               eps=eps, z_params=t(zp), z=t(z), noise=noise, y_mb=t(y_mb), y_raw=t(y_raw), cot_mb=c_mb, grads=grads)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", len(grads), "gradients")


def golden_v1_tiny(name="v1_tiny.pt"):
    """configs/v1.gin generator side: v1 Encoder (BatchNorm1d in training mode, grouped head conv),
    Generator (UpsampleLayer / ResidualStack, waveform x loudness, NoiseGenerator once warmed up).
    Forward products (noise draw captured) and parameter gradients under a fixed cotangent."""
    cap, lat, n_signal, batch = 4, 8, 8192, 3
    torch.manual_seed(0)
    m = build_reference_rave("v1", capacity=cap, latent_size=lat)
    m.train()
    sd = {k: t(v) for k, v in m.state_dict().items() if k.startswith(("pqmf.", "encoder.", "decoder."))}
    x = O.synthetic_batch(batch, 1, n_signal, seed=12)
    gen = torch.Generator().manual_seed(123)
    zp, x_mb = m.encode(x, return_mb=True)
    eps = torch.randn(zp.shape[0], lat, zp.shape[-1], generator=gen)
    mean, scale = zp.chunk(2, 1)
    z = eps * (torch.nn.functional.softplus(scale) + 1e-4) + mean
    y_cold = m.decoder(z)                                  # warmed_up == 0: no noise branch
    m.decoder.set_warmed_up(True)
    torch.manual_seed(999)
    y_warm = m.decoder(z)
    l_amp = y_warm.shape[-1] // 64                         # NoiseGenerator ratios [4,4,4]
    torch.manual_seed(999)
    noise = torch.rand(batch, l_amp, 16, 64) * 2 - 1
    c_mb = torch.randn(y_warm.shape, generator=gen)
    m.zero_grad(set_to_none=True)
    torch.autograd.backward([y_warm], [c_mb])
    grads = {k: t(p.grad) for k, p in m.named_parameters()
             if p.grad is not None and k.startswith(("encoder.", "decoder."))}
    out = dict(config=dict(capacity=cap, latent_size=lat, n_signal=n_signal, batch=batch), state_dict=sd, x=t(x),
               eps=eps, z_params=t(zp), z=t(z), y_cold=t(y_cold), y_warm=t(y_warm), noise=noise, cot_mb=c_mb,
               grads=grads)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", len(grads), "gradients", tuple(noise.shape))


def _subsample(g, step=257, keep=200_000):
    g = g.reshape(-1)
    return t(g) if g.numel() <= keep else t(g[::step])


def golden_disc2d(name="disc2d_tiny.pt"):
    """The reference's general-Conv2d discriminators on seeded inputs:
    (a) rave.discriminator.MultiScaleSpectralDiscriminator + EncodecConvNet (spectral_discriminator.gin:6-17,
        capacity shrunk to 8, scales [512, 128]);
    (b) rave.descript_discriminator.DescriptDiscriminator (v3.gin), stereo, periods [3], fft_sizes [256] --
        channel widths are hard-coded upstream (8.5 M parameters per MPD), so the fixture carries the SEED of
        rave_oracle.seeded_state_dict instead of the weights.
    Stored: every feature map, dL/dx and parameter gradients (large ones subsampled every 257th element) of
    L = sum_f mean(f^2)."""
    from functools import partial
    from ref_import import import_reference
    import_reference()
    from rave import descript_discriminator as rdd, discriminator as rd
    out = {}

    def run(model, x, seed, key, store_sd):
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(".window")}
        sd = O.seeded_state_dict(shapes, seed)
        missing = model.load_state_dict(sd, strict=False)
        assert all(k.endswith(".window") for k in missing.missing_keys) and not missing.unexpected_keys
        x = x.clone().requires_grad_(True)
        feats = model(x)
        flat = [f for net in feats for f in net]
        loss = sum(f.pow(2).mean() for f in flat)
        model.zero_grad(set_to_none=True)
        loss.backward()
        out[key] = dict(seed=seed, shapes=shapes, x=t(x), loss=t(loss), dx=t(x.grad),
                        features=[[t(f) for f in net] for net in feats],
                        grads={k: _subsample(p.grad) for k, p in model.named_parameters()},
                        grad_step=257)
        if store_sd:
            out[key]["state_dict"] = {k: t(v) for k, v in sd.items()}
        print(key, "loss", float(loss), "features", [len(n) for n in feats],
              "params", sum(p.numel() for p in model.parameters()))

    torch.manual_seed(0)
    enc = rd.MultiScaleSpectralDiscriminator(scales=[512, 128], convnet=partial(rd.EncodecConvNet, capacity=8),
                                             n_channels=1)
    run(enc, O.synthetic_batch(2, 1, 4096, seed=31), 101, "encodec", True)
    out["encodec"]["config"] = dict(scales=[512, 128], capacity=8, n_channels=1)
    des = rdd.DescriptDiscriminator(periods=[3], fft_sizes=[256], n_channels=2)
    run(des, O.synthetic_batch(1, 2, 2048, seed=32), 202, "descript", False)
    out["descript"]["config"] = dict(periods=[3], fft_sizes=[256], n_channels=2)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


def golden_rvq(name="rvq_tiny.pt"):
    """rave.quantization.ResidualVectorQuantization (discrete.gin:37-40 shrunk): k-means initialisation on a
    first batch (reference code, CPU RNG), then ONE training forward/backward and one eval forward on a second
    batch: outputs, commitment loss, indices, dL/dz and the EMA-updated codebook buffers."""
    from ref_import import import_reference
    import_reference()
    from rave import quantization as rq
    out = {}
    for tag, (nq, dim, k, b, tl) in dict(small=(4, 16, 32, 3, 40), wide=(3, 64, 256, 4, 128)).items():
        torch.manual_seed(5)
        m = rq.ResidualVectorQuantization(num_quantizers=nq, dim=dim, codebook_size=k)
        m.train()
        gen = torch.Generator().manual_seed(17)
        with torch.no_grad():
            m(torch.randn(b, dim, tl, generator=gen))         # k-means init + first EMA step
        sd0 = {kk: t(v) for kk, v in m.state_dict().items()}
        z = torch.randn(b, dim, tl, generator=gen).requires_grad_(True)
        q, loss, ind = m(z)
        cot = torch.randn(q.shape, generator=gen)
        ((q * cot).sum() + 3.0 * loss).backward()
        sd1 = {kk: t(v) for kk, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            q_eval, loss_eval, ind_eval = m(z.detach())
        out[tag] = dict(config=dict(num_quantizers=nq, dim=dim, codebook_size=k), sd0=sd0, z=t(z), cot=cot,
                        q=t(q), loss=t(loss), ind=t(ind), dz=t(z.grad), sd1=sd1, q_eval=t(q_eval),
                        loss_eval=t(loss_eval), ind_eval=t(ind_eval))
        print(tag, "loss", float(loss.detach()), "codes used", int(ind.unique().numel()))
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


def golden_v3_step_tiny(name="v3_step_tiny.pt"):
    """BASELINE configs[4] shrunk (configs/v3.gin + causal.gin, stereo): ONE discriminator step and ONE generator step
    of the reference's own ``training_step`` (rave/model.py:288-413) with the descript discriminator, from the same
    initial weights.  The discriminator's 42.6 M weights come from rave_oracle.seeded_state_dict (seed stored); stored
    are every logged loss and, for the discriminator step, the (subsampled) discriminator parameter gradients -- the
    hinge loss is well conditioned, unlike the spectral-loss gradient of the generator step."""
    cap, lat, n_signal, batch = 6, 8, 32768, 1
    torch.manual_seed(0)
    m = build_reference_rave("v3", n_channels=2, capacity=cap, latent_size=lat, causal=True)
    m.train()
    attach_optimizers(m)
    dshapes = {k: tuple(v.shape) for k, v in m.discriminator.state_dict().items() if not k.endswith(".window")}
    seed = 303
    m.discriminator.load_state_dict(O.seeded_state_dict(dshapes, seed), strict=False)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen_sd = {k: t(v) for k, v in init.items() if k.startswith(("pqmf.", "encoder.", "decoder."))}
    x = O.synthetic_batch(batch, 2, n_signal, seed=7)
    with torch.no_grad():
        zp = m.encode(x)
        torch.manual_seed(1234)
        z = m.encoder.reparametrize(zp)[0]
        torch.manual_seed(1234)
        eps = torch.randn(z.shape)
    out = dict(config=dict(capacity=cap, latent_size=lat, n_signal=n_signal, batch=batch, n_channels=2, causal=True),
               state_dict=gen_sd, disc_seed=seed, disc_shapes=dshapes, x=t(x), eps=eps, grad_step=257)
    for idx, tag in ((0, "dis"), (1, "gen")):
        m.load_state_dict(init)
        attach_optimizers(m)
        m.zero_grad(set_to_none=True)
        m.warmed_up = True
        torch.manual_seed(1234)
        m.training_step(x.clone(), idx)
        out[tag] = dict(losses={k: t(v) for k, v in m.logged.items() if torch.is_tensor(v)})
        if tag == "dis":
            out[tag]["grads"] = {k: _subsample(p.grad) for k, p in m.discriminator.named_parameters()}
        print(tag, {k: float(v) for k, v in out[tag]["losses"].items()})
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")
    build_reference_rave("v2", capacity=cap, latent_size=lat, causal=False)     # reset the causal gin binding


def golden_discrete_step_tiny(name="discrete_step_tiny.pt"):
    """BASELINE configs[3] shrunk (configs/discrete.gin + spectral_discriminator.gin, RVQ ENABLED as the benchmark
    does): k-means init + one warm-up pass by the reference, then ONE discriminator step and ONE generator step of its
    own ``training_step`` from the same state: every logged loss, the noise-augmentation draw (captured from
    torch.randn), the EMA-updated codebooks, and the discriminator gradients of the discriminator step."""
    cfg = dict(capacity=6, latent_size=8, noise_augmentation=4, num_quantizers=3, codebook_size=16, spectral_capacity=4)
    n_signal, batch = 32768, 2
    torch.manual_seed(0)
    m = build_reference_discrete(**cfg)
    m.train()
    attach_optimizers(m)
    m.encoder.enabled.fill_(1)
    x = O.synthetic_batch(batch, 1, n_signal, seed=11)
    with torch.no_grad():
        # default-initialised encoders emit |z| ~ 1e-3, which makes the commitment loss ~1e-8: raise the gain of the
        # head conv so that the quantiser works on O(1) latents
        head = [mod for mod in m.encoder.encoder.net if hasattr(mod, "weight_g")][-1]
        head.weight_g.mul_(300.0)
    with torch.no_grad():                       # k-means initialisation of every codebook + first EMA pass
        m.encoder.reparametrize(m.encode(x))
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out = dict(config=dict(cfg, n_signal=n_signal, batch=batch), state_dict={k: t(v) for k, v in init.items()}, x=t(x),
               grad_step=257)
    real_randn = torch.randn
    for idx, tag in ((0, "dis"), (1, "gen")):
        m.load_state_dict(init)
        attach_optimizers(m)
        m.zero_grad(set_to_none=True)
        m.warmed_up = True
        draws = []

        def spy(*a, **k):
            r = real_randn(*a, **k)
            draws.append(r.clone())
            return r

        torch.manual_seed(1234)
        torch.randn = spy
        try:
            m.training_step(x.clone(), idx)
        finally:
            torch.randn = real_randn
        noise = [d for d in draws if d.dim() == 3 and d.shape[1] == cfg["noise_augmentation"]]
        assert len(noise) == 1, [tuple(d.shape) for d in draws]
        out[tag] = dict(losses={k: t(v) for k, v in m.logged.items() if torch.is_tensor(v)}, noise=noise[0],
                        codebooks={k: t(v) for k, v in m.state_dict().items() if "_codebook" in k})
        if tag == "dis":
            out[tag]["grads"] = {k: _subsample(p.grad) for k, p in m.discriminator.named_parameters()}
        print(tag, {k: round(float(v), 5) for k, v in out[tag]["losses"].items()})
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")



def golden_v2_wide(name="v2_wide.pt"):
    """BASELINE configs[1] at its REAL width (v2.gin: CAPACITY 96, latent 128 -- 31.5 M generator-side weights,
    every conv at the channel count the benchmark runs), short clips (2 x 8192 samples): the reference's own
    encode -> reparametrize -> decode and its autograd backward under seeded cotangents at y_raw / y_mb (+ the KL
    term).  The weights come from rave_oracle.seeded_state_dict (the fixture carries the SEED); stored are the
    outputs, every weight_g gradient in full and every weight_v gradient subsampled (every 257th element).
    This is the fixture that reaches the bf16x6 kernels and the C = 768 / 1536 weight gradients with
    reference-produced numbers (the CAPACITY-6 fixtures never do)."""
    seed, batch, n_signal = 303, 2, 8192
    torch.manual_seed(0)
    m = build_reference_rave("v2", capacity=96, latent_size=128)
    m.train()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(("encoder.", "decoder."))}
    sd = O.seeded_state_dict(shapes, seed)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not any(k in sd for k in res.missing_keys)
    assert all(k in sd for k, _ in m.named_parameters() if k.startswith(("encoder.", "decoder.")))
    x = O.synthetic_batch(batch, 1, n_signal, seed=5)
    g = torch.Generator().manual_seed(17)
    zp, x_mb = m.encode(x, return_mb=True)
    torch.manual_seed(1234)
    z, reg = m.encoder.reparametrize(zp)[:2]
    torch.manual_seed(1234)
    eps = torch.randn(z.shape)
    y_mb = m.decoder(z)
    y_raw = m.decode(z)[..., :n_signal]
    cy_raw = torch.randn(y_raw.shape, generator=g) * 1e-3
    cy_mb = torch.randn(y_mb.shape, generator=g) * 1e-3
    m.zero_grad(set_to_none=True)
    torch.autograd.backward([y_raw, y_mb, reg], [cy_raw, cy_mb, torch.ones(())])
    grads = {}
    for k, p in m.named_parameters():
        if k.startswith(("encoder.", "decoder.")) and p.grad is not None:
            grads[k] = t(p.grad) if k.endswith("weight_g") else _subsample(p.grad, keep=20_000)
    # the same step by the same reference modules in float64: weight-norm gain gradients are sums with heavy
    # cancellation, so two fp32 implementations differ by up to ~1e-3 on a few of them; the parity tests judge
    # the HIP gradient against this value with the reference's own fp32 deviation as the yardstick
    m.double()
    m.zero_grad(set_to_none=True)
    zp64, _ = m.encode(x.double(), return_mb=True)
    mean, scale = zp64.chunk(2, 1)
    std = torch.nn.functional.softplus(scale) + 1e-4
    z64 = eps.double() * std + mean
    reg64 = (mean * mean + std * std - 2 * std.log() - 1).sum(1).mean()
    y_mb64 = m.decoder(z64)
    y_raw64 = m.decode(z64)[..., :n_signal]
    torch.autograd.backward([y_raw64, y_mb64, reg64], [cy_raw.double(), cy_mb.double(), torch.ones((), dtype=torch.float64)])
    assert abs(float(reg64) - float(reg)) < 1e-4 * abs(float(reg))
    grads64 = {}
    for k, p in m.named_parameters():
        if k.startswith(("encoder.", "decoder.")) and p.grad is not None:
            grads64[k] = t(p.grad) if k.endswith("weight_g") else _subsample(p.grad, keep=20_000)
    m.float()
    out = dict(grads64=grads64, config=dict(capacity=96, latent_size=128, n_signal=n_signal, batch=batch), seed=seed, shapes=shapes,
               x=t(x), eps=eps, x_mb=t(x_mb), z_params=t(zp), z=t(z), reg=t(reg), y_mb=t(y_mb), y_raw=t(y_raw),
               cot_y_raw=cy_raw, cot_y_mb=cy_mb, grads=grads, grad_step=257, grad_keep=20_000)
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", len(grads), "gradients; reg", float(reg))


def golden_reference_checks(name="reference_checks.pt"):
    """Outputs of the reference's own classes that tests/test_oracle.py and tests/test_abi_and_host.py compare the oracle
    and the drop-in modules with: the v2 modules (both paddings), the polyphase / classic PQMF forms, the spectral and
    Encodec distances and the latent-space wrappers."""
    from functools import partial
    from ref_import import import_reference
    import_reference()
    from rave import blocks as rb, core, pqmf as rp
    out = {}
    # seeded weights (O.seeded_state_dict): the fixture carries the seed, the shapes and the weight_g tensors (a norm
    # reduction whose last bits may depend on the host).  Inputs are stored whole; outputs above `keep` elements as a fixed
    # strided sample (_subsample): every `out_step`-th element, every `step`-th of a discriminator feature map
    seed, step, keep, out_step = 3, 61, 2048, 3
    out_keep = 4 * keep
    sub = lambda v: _subsample(v, out_step, out_keep)
    for causal in (False, True):
        torch.manual_seed(3)
        m = build_reference_rave("v2", capacity=10, latent_size=12, causal=causal)
        m.train()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()
                  if k.startswith(("encoder.", "decoder.", "discriminator.")) and k.endswith((".weight_v", ".weight_g", ".weight", ".bias"))}
        sd = O.seeded_state_dict(shapes, seed)
        missing = set(m.state_dict()) - set(sd)
        m.load_state_dict(sd, strict=False)
        assert all(k.startswith(("pqmf.", "audio_distance.", "multiband_audio_distance.", "latent_", "fidelity", "receptive_field",
                                 "encoder.warmed_up")) for k in missing), sorted(missing)
        x = O.synthetic_batch(2, 1, 8192, seed=9)
        with torch.no_grad():
            zp, xmb = m.encode(x, return_mb=True)
            eps = torch.randn(2, 12, zp.shape[-1])
            z, _ = O.reparametrize(zp, eps)
            y_mb = m.decoder(z)
            yr = m.decode(z)
            feats = m.discriminator(torch.cat([x, yr], 0))
            dist = m.audio_distance(x, yr)["spectral_distance"]
        rec = dict(x_mb=sub(xmb), z_params=t(zp), z=t(z), y_mb=sub(y_mb), y_raw=sub(yr),
                   feature_shapes=[[tuple(f.shape) for f in net] for net in feats],
                   features=[[_subsample(f, step, keep) for f in net] for net in feats], spectral_distance=t(dist))
        if not causal:
            rec.update(x=t(x), seed=seed, shapes=shapes, feature_step=step, feature_keep=keep, out_step=out_step, out_keep=out_keep,
                       weight_g={k: t(v) for k, v in sd.items() if k.endswith(".weight_g")})
        out["modules_causal" if causal else "modules"] = rec
    build_reference_rave("v2", capacity=4, latent_size=4, causal=False)  # reset the causal binding

    b = O.pqmf_buffers(100, 16)
    x = O.synthetic_batch(2, 1, 4096, seed=1)
    out["pqmf_forms"] = dict(x=t(x), polyphase=t(rp.reverse_half(rp.polyphase_forward(x, b["hk"]))),
                             classic=t(rp.reverse_half(rp.classic_forward(x, b["hk"]))))
    hk = b["hk"]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 4096, generator=g)
    y = torch.randn(2, 16, 256, generator=g)
    forms = {}
    for poly in (True, False):
        m = rp.PQMF(attenuation=100, n_band=16, polyphase=poly)
        with torch.no_grad():
            forms["polyphase" if poly else "classic"] = dict(forward=t(m(x)), inverse=t(m.inverse(y)))
    out["pqmf_noncached"] = dict(x=t(x), y=t(y), **forms)

    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, 6000, generator=g)
    y = (x + 0.1 * torch.randn(2, 1, 6000, generator=g))
    dists = {}
    for power, normalized, norms in ((1, True, ("L1", "L2")), (2, False, "L2"), (None, True, "L1")):
        kw = dict(sampling_rate=44100, norm=norms, power=power, normalized=normalized)
        rec = {}
        for n_fft in (256, 1024):
            ya = y.clone().requires_grad_(True)
            da = core.SpectralDistance(n_fft, **kw)(x, ya)
            da.backward()
            rec[n_fft] = dict(distance=t(da), grad_y=sub(ya.grad))
        ra = core.EncodecAudioDistance([256, 512], partial(core.SpectralDistance, **kw))(x, y)
        rec["encodec"] = {k: t(v) for k, v in ra.items()}
        dists[(power, normalized, norms)] = rec
    out["distances"] = dict(x=t(x), y=t(y), cases=dists, out_step=out_step, out_keep=out_keep)

    enc = lambda n_channels=1: torch.nn.Identity()
    z = torch.randn(3, 8, 16, generator=torch.Generator().manual_seed(5))
    w = rb.WasserteinEncoder(enc, noise_augmentation=0)
    torch.manual_seed(1)
    zw, rw = w.reparametrize(z)
    d = rb.DiscreteEncoder(enc, vq_cls=lambda: torch.nn.Identity(), num_quantizers=16, noise_augmentation=4)
    torch.manual_seed(2)
    zd, rd = d.reparametrize(z)
    out["latent"] = dict(z=t(z), wasserstein=(t(zw), t(rw)), spherical=t(rb.SphericalEncoder(enc).reparametrize(z)[0]),
                         discrete=(t(zd), float(rd)), discrete_state_keys=sorted(d.state_dict()))
    torch.save(out, os.path.join(OUT, name))
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    golden_pqmf()
    golden_v2_tiny(False, "v2_tiny.pt")
    golden_v2_tiny(True, "v2_tiny_causal.pt")
    golden_v3_gen_tiny()
    golden_v2_small_tiny()
    golden_v1_tiny()
    golden_disc2d()
    golden_rvq()
    golden_v3_step_tiny()
    golden_discrete_step_tiny()
    golden_v2_wide()
    golden_v3_validation_tiny()
    golden_reference_checks()
