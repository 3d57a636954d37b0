"""Parameter gradients land where a data-parallel reducer puts them: in views of one flat buffer that are only 4-byte aligned.

rave_amd.ddp.GradReducer lays the parameters of a model back to back (no padding) and the backward kernels write dw / dbias /
dv / dg straight into those views (rave_amd.ops._grad_out).  The discriminators end in a one-element bias, so in multi-GPU
GAN-phase training most gradient views start 1, 2 or 3 floats off a 16-byte boundary (tests/test_misaligned_host.py pins that);
every other test of the suite hands the kernels 512-byte aligned tensors of the caching allocator.

Every test here runs forward + backward from identical inputs under fixed cotangents, first without a reducer (fresh, aligned
gradient tensors) and then with a reducer whose views are shifted by 1, 2 and 3 floats -- one dummy parameter of ``shift``
elements goes last into the parameter list, i.e. first into the bucket.  One process, no process group (misaligned.py:
bucket_reducer).  Asserted per run: the adopted gradient IS the bucket view and has the address residue it claims; every
gradient is finite, within the tolerance of the corresponding aligned test against an f64 evaluation on the CPU, and
``torch.equal`` to the aligned run; the two dummy slots that enclose the views in the flat buffer keep their guard pattern; a
second run gives the same bits.  No case had to be relaxed from bit-equality: at these sizes no host line selects another
summation order for a misaligned pointer (reduce_is_vec4, conv_wgrad.hip, needs >= 65536 elements).
"""
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import rave_oracle as O
from conftest import rel_l2
from misaligned import _Env, bucket_reducer, fill_guard, is_guard
from test_gpu_parity import TOL_E2E, TOL_OP
from test_gpu_wgrad_wide import CLEAN, _plan


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def _grads(params):
    return [None if p.grad is None else p.grad.detach().clone() for p in params]


def _check_under_shifted_buckets(dev, named, run, want64, tol, env=None, expect_packed=()):
    """``named``: {name: parameter}; ``run()``: forward + backward (gradients were cleared before); ``want64``: {name: f64
    gradient}.  ``expect_packed``: name fragments of the parameters whose gradient torch ops produce (copied into the view
    by the reducer's hook, rave_amd.ddp: _on_grad) -- every other gradient must be WRITTEN into its view by the kernels; an
    int: that many gradient ELEMENTS take the copy (the general Conv2d operator, rave_amd.ops._Conv2dFn, returns fresh gradient
    tensors, which the hook copies: a change there shows as a change of this number)."""
    env = {**CLEAN, **(env or {})}
    names, params = list(named), list(named.values())

    def clear():
        for p in params:
            p.grad = None

    with _Env(**env):
        clear()
        run()
        torch.cuda.synchronize()
        base = _grads(params)
    worst_base = 0.0
    for k, g in zip(names, base):
        assert g is not None and torch.isfinite(g).all(), k
        assert g.data_ptr() % 16 == 0
        worst_base = max(worst_base, rel_l2(g, want64[k]))
    seen = set()
    for shift in (1, 2, 3):
        tail = nn.Parameter(torch.zeros(64, device=dev))            # first in the list = last in the flat buffer
        head = nn.Parameter(torch.zeros(shift, device=dev))         # last in the list = offset 0 of the flat buffer
        red = bucket_reducer([tail] + params + [head], bucket_mb=1024.0, tail_mb=0.0)      # one bucket, nothing peeled off
        assert len(red.buckets) == 1
        b = red.buckets[0]
        assert b.flat.data_ptr() % 16 == 0 and b.views[0].data_ptr() == b.flat.data_ptr() and b.params[0] is head
        assert b.params[-1] is tail and b.views[-1].storage_offset() + 64 == b.flat.numel()
        assert b.views[1].data_ptr() % 16 == 4 * shift               # the first real view: `shift` floats off the boundary
        fill_guard(b.views[0]); fill_guard(b.views[-1])
        runs = []
        with _Env(**env):
            for rep in range(2):
                clear()
                b.flat[shift:-64].zero_()
                red.begin()
                run()
                red.finish()
                torch.cuda.synchronize()
                for k, p in named.items():
                    v = b.views[b.index[p]]
                    assert p.grad is not None and p.grad.data_ptr() == v.data_ptr(), k          # the gradient IS the view
                    assert p.grad.data_ptr() % 16 == 4 * (v.storage_offset() % 4)
                    if v.numel() >= 64:
                        seen.add((shift, v.storage_offset() % 4))
                runs.append(_grads(params))
                assert is_guard(b.views[0]) and is_guard(b.views[-1]), (shift, rep)    # nothing written outside the views
        packed = red.bytes_packed
        if isinstance(expect_packed, int):         # a stack of Conv2d operators: so many gradient elements take the copy
            print(f"shift {shift}: {packed // 8} of {sum(p.numel() for p in params)} gradient elements were copied into their view")
            assert packed == 8 * expect_packed, (packed // 8, expect_packed)
        else:
            want_packed = 4 * sum(p.numel() for k, p in named.items() if any(f in k for f in expect_packed))
            assert packed == 2 * want_packed, (packed, want_packed)
        red.remove()
        worst = 0.0
        for k, g0, g1, g2 in zip(names, base, runs[0], runs[1]):
            assert torch.isfinite(g1).all(), (k, shift)
            e = rel_l2(g1, want64[k])
            worst = max(worst, e)
            assert e < tol, (k, shift, e, rel_l2(g0, want64[k]))
            assert torch.equal(g1, g0), (k, shift, rel_l2(g1, g0))
            assert torch.equal(g2, g1), (k, shift, "second run")
        print(f"shift {shift}: worst rel-L2 against f64 {worst:.2e} (aligned run {worst_base:.2e}, bound {tol:.0e}); "
              f"all {len(names)} gradients bit-identical to the aligned run")
    assert worst_base < tol
    # under every shift a large gradient tensor sat `shift` floats off a 16-byte boundary
    assert {(1, 1), (2, 2), (3, 3)} <= seen, seen


def _seeded(model, seed, dev):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(".window")}
    sd = O.seeded_state_dict(shapes, seed)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".window") for k in res.missing_keys)
    model.to(dev).train()
    return sd


def _feature_cots(feats, seed):
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(f.shape, generator=gen) / f.numel() ** 0.5 for f in net] for net in feats]


def _disc_case(dev, model, ref_fn, x, env=None, expect_packed=()):
    sd = _seeded(model, 11, dev)
    leaves64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f64 = ref_fn(x.double(), leaves64)
    cots = _feature_cots(f64, 5)
    torch.autograd.backward([f for net in f64 for f in net], [c.double() for net in cots for c in net])
    want = {k: v.grad for k, v in leaves64.items() if v.grad is not None}
    xg = x.to(dev)
    cg = [c.to(dev) for net in cots for c in net]

    def run():
        feats = model(xg)
        assert [tuple(f.shape) for net in feats for f in net] == [tuple(c.shape) for c in cg]
        torch.autograd.backward([f for net in feats for f in net], cg)

    named = dict(model.named_parameters())
    assert set(named) == set(want)
    _check_under_shifted_buckets(dev, named, run, want, TOL_E2E, env, expect_packed)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["identity", "weight_norm"])
def test_v2_discriminator_gradients_in_misaligned_bucket_views(dev, mode, monkeypatch):
    """rave_amd.discriminator MultiPeriodDiscriminator (periods 2, 3: the (5,1) Conv2d form with inner > 1) +
    MultiScaleDiscriminator, capacity 16, 3 layers, 2 x 4111 samples.  ``identity``: no weight norm, so dw / dbias of
    rh_conv1d_bwd_weight_f32 (first-layer vector kernels, the matrix-core paths) and rh_act_bwd_bias_f32 are written into the
    views themselves; ``weight_norm`` (what the shipped configs use): dv / dg of the weight-norm backward are."""
    from rave_amd import blocks
    from rave_amd import discriminator as D
    cfg = O.v2_config(periods=(2, 3), disc_layers=3)
    common = dict(out_size=1, capacity=16, n_layers=3, stride=4)
    monkeypatch.setattr(blocks, "_NORMALIZATION_MODE", mode)
    mpd = partial(D.MultiPeriodDiscriminator, periods=[2, 3], convnet=partial(D.ConvNet, conv=nn.Conv2d, kernel_size=(5, 1), **common))
    msd = partial(D.MultiScaleDiscriminator, n_discriminators=3, convnet=partial(D.ConvNet, conv=nn.Conv1d, kernel_size=15, **common))
    model = D.CombineDiscriminators(discriminators=[mpd, msd], n_channels=1)
    if mode == "identity":       # the oracle's nets are weight-normed: hand it the plain weight in place of (v, g)
        wn = O.weight_norm
        monkeypatch.setattr(O, "weight_norm", lambda v, g: v if g is None else wn(v, g))

    def ref(x, sd):
        full = {"discriminator." + k: v for k, v in sd.items()}
        if mode == "identity":
            for k in list(full):
                if k.endswith(".weight"):
                    full[k + "_v"], full[k + "_g"] = full[k], None
        return O.combine_discriminators(x, full, cfg)

    _disc_case(dev, model, ref, O.synthetic_batch(2, 1, 4111, seed=41))


@pytest.mark.gpu
@pytest.mark.parametrize("x6", ["1", "0"])
def test_encodec_spectral_discriminator_gradients_in_misaligned_bucket_views(dev, x6):
    """Encodec STFT nets at the widths of tests/golden/disc2d_tiny.pt: rh_conv2d_bwd_weight_f32 on the f16-piece kernel
    (RH_CONV2D_X6=1) and on the f32 kernels (0), weight-normalised Conv2d.  The general Conv2d operator does not write into
    gradient slots: its gradients reach the misaligned views through the reducer's copy (printed), so what this pins is that
    copy and the values; rh_conv2d_bwd_weight_f32 itself never sees a bucket view today."""
    from rave_amd import discriminator as D
    scales = [512, 128]
    model = D.MultiScaleSpectralDiscriminator(scales, partial(D.EncodecConvNet, capacity=8), n_channels=1)
    _disc_case(dev, model, lambda x, sd: O.multiscale_spectral_discriminator(x, {"d." + k: v for k, v in sd.items()}, "d", scales),
               O.synthetic_batch(2, 1, 4096, seed=43), env=dict(RH_CONV2D_X6=x6), expect_packed=12692)         # every parameter of the stack


@pytest.mark.gpu
@pytest.mark.parametrize("x6", ["1", "0"])
def test_descript_discriminator_gradients_in_misaligned_bucket_views(dev, x6):
    """Descript MPD (period 3) + MRD (fft 256), stereo, at the widths of tests/golden/disc2d_tiny.pt."""
    from rave_amd import descript_discriminator as DD
    model = DD.DescriptDiscriminator(periods=[3], fft_sizes=[256], n_channels=2)
    _disc_case(dev, model, lambda x, sd: O.descript_discriminator(x, {"d." + k: v for k, v in sd.items()}, "d", [3], [256]),
               O.synthetic_batch(1, 2, 2048, seed=45), env=dict(RH_CONV2D_X6=x6), expect_packed=479970)      # the MRD's Conv2d nets


GEN_ENVS = {
    "side_stream_collected": dict(),                                    # collected weight-norm backward at the join (default)
    "side_stream_deferred_reductions": dict(RH_REDUCE_BATCH=8),         # + the batched reduction a recorded step uses
    "one_call_two_launches": dict(RH_BWD_SIDE_STREAM=0, RH_WN_FUSED=0),  # rh_conv1d_bwd_weight_wn_f32
    "one_call_fused_launch": dict(RH_BWD_SIDE_STREAM=0, RH_WN_FUSED=1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(GEN_ENVS), ids=list(GEN_ENVS))
def test_v2_generator_gradients_in_misaligned_bucket_views(dev, env):
    """The v2 encoder + decoder at capacity 16 on 4 x 4096 samples: dv / dg of every weight-normed conv through the collected
    weight-norm backward of the side stream (with and without deferred batched reductions) and through
    rh_conv1d_bwd_weight_wn_f32 in its two- and one-launch form."""
    from rave_amd import model as M
    cfg = O.v2_config(capacity=16, latent_size=16)
    sd = O.init_state_dict(cfg, seed=0)
    m = M.build_v2(capacity=16, latent_size=16)
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).train()
    x = O.synthetic_batch(4, 1, 4096, seed=9)
    eps = torch.randn(4, 16, 2, generator=torch.Generator().manual_seed(3))
    leaves64 = {k: (v.double().requires_grad_(True) if k.startswith(("encoder.", "decoder.")) else v.double()) for k, v in sd.items()
                if v.is_floating_point()}
    out = O.rave_forward(x.double(), leaves64, cfg, eps.double())
    gen = torch.Generator().manual_seed(17)
    c_mb = torch.randn(out["y_mb"].shape, generator=gen) / out["y_mb"].numel() ** 0.5
    torch.autograd.backward([out["y_mb"], out["reg"]], [c_mb.double(), torch.ones((), dtype=torch.float64)])
    named = {k: p for k, p in m.named_parameters() if k.startswith(("encoder.", "decoder."))}
    want = {k: leaves64[k].grad for k in named}
    xg, eg, cg = x.to(dev), eps.to(dev), c_mb.to(dev)

    def run():
        zp = m.encode(xg)
        z, reg = m.encoder.reparametrize(zp, eg)
        y_mb = m.decoder(z)
        torch.autograd.backward([y_mb[..., :cg.shape[-1]], reg], [cg, torch.ones((), device=dev)])

    _check_under_shifted_buckets(dev, named, run, want, TOL_E2E, GEN_ENVS[env])


WN_CONVS = [
    # (name, c_in, c_out, k, dilation, waves of the plan)       B = 2, L = 512
    ("rows96_cols288_wide_tile", 96, 96, 3, 3, 9),
    ("rows192_cols288_four_wave_tile", 96, 192, 3, 1, 4),
]


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["1", "0"])
@pytest.mark.parametrize("case", WN_CONVS, ids=[c[0] for c in WN_CONVS])
def test_split_k_weight_gradient_of_a_weight_normed_conv_in_misaligned_views(dev, case, side):
    """One weight-normed conv whose K range is really cut into slices (RH_WGRAD_X6_BLOCKS=1024; asserted from
    rh_conv1d_bwd_weight_plan_info): the ordered reduction and the weight-norm backward behind the column-complete tile (96
    rows, 288 columns) and behind the 4-wave tile (192 rows) write dv / dg / dbias into misaligned views."""
    from rave_amd import ops as R
    name, c_in, c_out, k, dil, waves = case
    B, L = 2, 512
    kw = dict(dilation=dil, pad_left=dil, pad_right=dil, act=1, slope=0.2)
    env = dict(RH_WGRAD_X6_BLOCKS=1024, RH_BWD_SIDE_STREAM=side)
    plan = _plan((name, B, c_in, c_out, L, k, kw, waves), RH_WGRAD_X6_BLOCKS=1024)
    assert plan["slices"] > 1 and plan["waves"] == waves, plan
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(B, c_in, L, generator=gen)
    v0 = torch.randn(c_out, c_in, k, generator=gen) * 0.05
    g0 = torch.rand(c_out, 1, 1, generator=gen) + 0.5
    b0 = torch.randn(c_out, generator=gen)
    cot = torch.randn(B, c_out, L, generator=gen)
    v64, g64, b64 = (t.double().requires_grad_(True) for t in (v0, g0, b0))
    y64 = F.conv1d(F.leaky_relu(x.double(), 0.2), O.weight_norm(v64, g64), b64, 1, dil, dil)
    y64.backward(cot.double())
    named = {"weight_v": nn.Parameter(v0.to(dev)), "weight_g": nn.Parameter(g0.to(dev)), "bias": nn.Parameter(b0.to(dev))}
    want = {"weight_v": v64.grad, "weight_g": g64.grad, "bias": b64.grad}
    geom = R.ConvGeom(**kw)
    xg, cg = x.to(dev), cot.to(dev)

    def run():
        y = R.conv1d(xg, named["weight_v"], named["bias"], geom=geom, weight_g=named["weight_g"])
        y.backward(cg)

    _check_under_shifted_buckets(dev, named, run, want, TOL_OP, env)


@pytest.mark.gpu
def test_snake_unit_gradients_in_misaligned_bucket_views(dev, monkeypatch):
    """A v3-style residual unit (Snake -> weight-normed conv k3 d3 -> Snake -> weight-normed 1x1, skip added): the Snake alphas'
    gradients come from rh_snake_bwd_f32 through autograd and take the reducer's copy path (rave_amd.ddp: _on_grad), the
    convs' dv / dg are written in place."""
    from rave_amd import blocks
    monkeypatch.setattr(blocks, "_NORMALIZATION_MODE", "weight_norm")
    unit = blocks.Residual(blocks.DilatedUnit(32, 3, 3, activation=blocks.Snake))
    gen = torch.Generator().manual_seed(29)
    sd = {}
    for k, p in unit.named_parameters():
        sd[k] = torch.rand(p.shape, generator=gen) + 0.5 if k.endswith(("alpha", "weight_g")) else torch.randn(p.shape, generator=gen) * 0.1
    unit.load_state_dict(sd)
    unit.to(dev).train()
    x = torch.randn(2, 32, 301, generator=gen)
    cot = torch.randn(2, 32, 301, generator=gen)
    leaves64 = {"u." + k: v.double().requires_grad_(True) for k, v in sd.items()}
    y64 = O.dilated_unit_residual(x.double(), leaves64, "u", 3, O.v3_config(causal=False))
    y64.backward(cot.double())
    named = dict(unit.named_parameters())
    want = {k: leaves64["u." + k].grad for k in named}
    xg, cg = x.to(dev), cot.to(dev)

    def run():
        unit(xg).backward(cg)

    _check_under_shifted_buckets(dev, named, run, want, TOL_OP, expect_packed=("alpha",))
