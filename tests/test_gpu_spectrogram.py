"""GPU tests of the complex spectrogram (rave_amd/csrc/spectrogram.hip, rave_amd.ops.spectrogram, rave_amd.Spectrogram and the
``hip_frontend`` flag of the two spectral discriminators): forward and the adjoint against the float64 restatement of
tests/spectrogram_reference.py and float64 autograd through it, at the project's parity bar -- relative L2 <= 1e-4, the constant
tests/test_gpu_mel.py holds the same in-LDS transform to.  Measured on the MI355X over the cases below (per n_fft in
profiles/spectrogram.txt): forward 1.3e-7 .. 1.6e-7, backward 1.2e-7 .. 2.4e-7 (the largest at hop = 1)."""
import os
from functools import partial

import pytest
import torch

import spectrogram_reference as R
from conftest import rel_l2
from test_gpu_mel import BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _mod(n_fft, hop, center, dev, normalized=True):
    import rave_amd
    return rave_amd.Spectrogram(n_fft, hop_length=hop, power=None, normalized=normalized, center=center).to(dev)


# n_fft, hop, T: one frame; a tail that forms no frame; several frames; the packed-complex path; three tiles and three spans;
# an odd frame count at 2048; hop = n_fft and hop = 1
CASES = [(128, 32, 128), (256, 64, 256 + 64 * 5 + 17), (1024, 256, 1024 + 256 * 4), (4096, 1024, 4096 + 1024 * 2),
         (128, 32, 5000), (2048, 512, 2048 + 512 * 20), (128, 128, 128 * 5 + 3), (128, 1, 300)]
# The 16-byte path of the tile (float4 stores of `out`, float4 loads of `dout`) runs only where the frame count is a multiple of
# 4.  None of the above has one (1, 5, 9, 21, 25, 153, 157 ... frames), so one case per size below 4096 (which never takes it):
# T = n_fft + 19 hop gives 20 frames uncentred and 24 centred; the longer ones give 100 / 104 and 44 / 48 frames, more than the
# one tile of 64 / 32 frames at 128 / 256 (tiles of 16, 8 and 4 frames at 512, 1024, 2048: a partial last tile, 2 - 5 spans).
VEC4 = [(128, 32, 128 + 32 * 99), (256, 64, 256 + 64 * 43), (512, 128, 512 + 128 * 19), (1024, 256, 1024 + 256 * 19),
        (2048, 512, 2048 + 512 * 19)]
CASES += VEC4
SHORT = [(n, n // 4, n // 2 + 1) for n in (128, 256, 1024, 4096)]          # centred only: the shortest legal reflect
ALL = [(n, h, t, c) for n, h, t in CASES for c in (False, True)] + [(n, h, t, True) for n, h, t in SHORT]

_REF = {}


def _reference(n_fft, hop, t, center):
    """(x, g, window, planes of x, the adjoint applied to g) in float64, computed once per case and shared."""
    key = (n_fft, hop, t, center)
    if key not in _REF:
        x = R.white_noise((3, t), 11 + n_fft + t, torch.float64).requires_grad_(True)
        win = torch.hann_window(n_fft, dtype=torch.float64)
        s = R.planes(x, win, n_fft, hop, True, center)
        g = R.white_noise(tuple(s.shape), 12 + n_fft + t, torch.float64)
        (dx,) = torch.autograd.grad(s, x, g)
        _REF[key] = (x.detach(), g, win, s.detach(), dx)
    return _REF[key]


@pytest.mark.parametrize("n_fft,hop,t,center", ALL)
def test_forward_and_backward_against_float64(dev, n_fft, hop, t, center):
    x, g, win, s, dx = _reference(n_fft, hop, t, center)
    m = _mod(n_fft, hop, center, dev)
    frames = R.frames_of(n_fft, hop, t, center)
    bins = n_fft // 2 + 1
    for shape in ((3, 1, t), (1, 3, t)):                       # rows = 3 as (B=3, C=1) and as (B=1, C=3)
        b, c = shape[:2]
        xg = x.float().reshape(shape).to(dev).requires_grad_(True)
        got = m.real_imag(xg)
        # cat([real, imag], 1): channel p * C + c of batch b is plane p of row b * C + c
        want = s.reshape(b, c, 2, bins, frames).transpose(1, 2).reshape(b, 2 * c, bins, frames)
        gg = g.reshape(b, c, 2, bins, frames).transpose(1, 2).reshape(b, 2 * c, bins, frames)
        assert tuple(got.shape) == (b, 2 * c, bins, frames) and got.is_contiguous()
        ef = rel_l2(got, want)
        (dxg,) = torch.autograd.grad(got, xg, gg.float().to(dev))
        eb = rel_l2(dxg.reshape(3, t), dx)
        # <S x, g> == <x, S^T g> in float64 accumulation; either side is off by at most BAR of its own norms
        lhs = float((got.detach().double().cpu() * gg).sum())
        rhs = float((xg.detach().double().cpu().reshape(3, t) * dxg.double().cpu().reshape(3, t)).sum())
        slack = BAR * (float(want.norm() * gg.norm()) + float(x.norm() * dx.norm()))
        print(f"spectrogram n_fft {n_fft} hop {hop} T {t} center {center} (B, C) = ({b}, {c}): forward {ef:.2e}, backward {eb:.2e}, "
              f"adjoint identity off by {abs(lhs - rhs) / slack * BAR:.2e} of the norms")
        assert ef <= BAR and eb <= BAR
        assert abs(lhs - rhs) <= slack
    pl = m.planes(x.float().reshape(1, 3, t).to(dev))          # the (..., 2, bins, frames) layout and torchaudio's complex result
    assert tuple(pl.shape) == (1, 3, 2, bins, frames) and rel_l2(pl, s.reshape(1, 3, 2, bins, frames)) <= BAR
    z = m(x.float().to(dev))
    assert z.dtype == torch.complex64 and tuple(z.shape) == (3, bins, frames)
    assert torch.equal(z.real, pl[0, :, 0]) and torch.equal(z.imag, pl[0, :, 1])


@pytest.mark.parametrize("n_fft,hop,t,center", [(512, 128, 512 + 128 * 19, False), (128, 32, 5000, True), (4096, 1024, 4096 + 1024 * 2, True)])
def test_backward_gives_the_same_bits_five_times(dev, n_fft, hop, t, center):
    from rave_amd import ops
    x, g, win, s, dx = _reference(n_fft, hop, t, center)
    xg = x.float().to(dev).requires_grad_(True)
    gg = g.float().to(dev)
    winf = win.float().to(dev)
    runs = []
    for _ in range(5):
        out = ops.spectrogram(xg, winf, n_fft, hop, True, center)
        runs.append((out.detach().clone(), torch.autograd.grad(out, xg, gg)[0].clone()))
    for o, d in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(d, runs[0][1])


@pytest.mark.parametrize("power", [1, 2])
def test_power_spectrogram(dev, power):
    import rave_amd
    x, g, win, s, dx = _reference(256, 64, 256 + 64 * 5 + 17, True)
    m = rave_amd.Spectrogram(256, hop_length=64, power=power, normalized=True).to(dev)
    want = R.spectrogram(x, win, 256, 64, True, True, power)
    assert rel_l2(m(x.float().to(dev)), want) <= BAR


def test_a_loaded_window_is_honoured(dev):
    n_fft, hop, t = 256, 64, 1000
    m = _mod(n_fft, hop, False, dev)
    x = R.white_noise((2, 1, t), 21).to(dev)
    before = m.real_imag(x)                                                 # the Hann result, and its cached norm
    ham = torch.hamming_window(n_fft)
    m.load_state_dict({"window": ham})
    got = m.real_imag(x)
    want = R.real_imag(x.double().cpu(), ham.double(), n_fft, hop, True, False)
    assert rel_l2(got, want) <= BAR and rel_l2(before, want) > 1e-2
    with torch.no_grad():
        m.window.copy_(torch.hann_window(n_fft))                            # overwritten in place: the version counter moves
    assert torch.equal(m.real_imag(x), before)


@pytest.mark.parametrize("n_fft,hop,t,center", [(n, h, t, c) for n, h, t in VEC4 for c in (False, True)] +
                         [(4096, 1024, 4096 + 1024 * 2, True), (2048, 512, 2048 + 512 * 20, False)])
def test_pointers_that_are_only_4_byte_aligned(dev, n_fft, hop, t, center):
    """Offset views against 16-byte-aligned tensors, bit for bit.  At the VEC4 sizes the aligned call takes the float4 path of the
    tile and the offset ones the scalar path, so this also holds the two paths to the same bits; the last two cases (3 and 21
    frames) compare scalar with scalar."""
    import misaligned as MA
    from rave_amd import _lib as L, ops
    xr, g, win, s, dx = _reference(n_fft, hop, t, center)
    x, gg, w = xr.float().to(dev), g.float().to(dev), win.float().to(dev)
    tw = ops._twiddle(n_fft, dev)
    scale = ops.spectrogram_scale(w)

    def fwd(xv, wv, out):
        return L.lib.rh_spectrogram_fwd_f32(L.ptr(xv), L.ptr(wv), L.ptr(tw), 3, 1, t, n_fft, hop, int(center), scale, L.ptr(out), L.stream())

    def bwd(gv, wv, out):
        return L.lib.rh_spectrogram_bwd_f32(L.ptr(gv), L.ptr(wv), L.ptr(tw), 3, 1, t, n_fft, hop, int(center), scale, L.ptr(out), L.stream())

    base_o, base_d = torch.zeros_like(gg), torch.zeros_like(x)
    assert base_o.data_ptr() % 16 == 0 and gg.data_ptr() % 16 == 0
    assert fwd(x, w, base_o) == 0 and bwd(gg, w, base_d) == 0
    for off in (1, 2, 3):
        xs, ws, gs = MA.carve(x, off), MA.carve(w, (off + 1) % 4), MA.carve(gg, off)
        os_, ds = MA.carve(torch.zeros_like(gg), (off + 2) % 4 or 1), MA.carve(torch.zeros_like(x), off)
        assert fwd(xs, ws, os_) == 0 and bwd(gs, ws, ds) == 0
        torch.cuda.synchronize()
        assert torch.equal(os_, base_o) and torch.equal(ds, base_d), off
        assert all(MA.guards_intact(v) for v in (xs, ws, gs, os_, ds)), off


def _grads_match(on, off, x, feats_of):
    out = []
    for m in (on, off):
        xg = x.clone().requires_grad_(True)
        feats = feats_of(m, xg)
        sum(f.pow(2).mean() for net in feats for f in net).backward()
        out.append((xg.grad, feats))
    return out


def test_encodec_discriminator_with_the_flag(dev, golden_dir):
    """The (real, imag) planes of the kernel under the Encodec nets: features against the reference's recorded ones at the bar
    of tests/test_gpu_parity.py, gradients against the same model on torch.stft + cat."""
    from rave_amd import discriminator as D
    from test_gpu_parity import TOL_E2E
    g = torch.load(os.path.join(golden_dir, "disc2d_tiny.pt"), weights_only=False)["encodec"]
    c = g["config"]
    assert list(c["scales"]) == [512, 128] and c["capacity"] == 8
    on, off = (D.MultiScaleSpectralDiscriminator(c["scales"], partial(D.EncodecConvNet, capacity=c["capacity"]), n_channels=c["n_channels"],
                                                 hip_frontend=h) for h in (True, False))
    for m in (on, off):
        m.load_state_dict(g["state_dict"], strict=False)
        m.to(dev)
    (dx_on, feats), (dx_off, _) = _grads_match(on, off, g["x"].to(dev), lambda m, x: m(x))
    worst = max(rel_l2(f, gf) for net, gnet in zip(feats, g["features"]) for f, gf in zip(net, gnet))
    first = "nets.0.net.0.0.weight_v"
    w_on, w_off = dict(on.named_parameters())[first].grad, dict(off.named_parameters())[first].grad
    print(f"encodec, hip_frontend: features {worst:.2e} of the fixture; dx {rel_l2(dx_on, dx_off):.2e}, d {first} {rel_l2(w_on, w_off):.2e} "
          "of the torch.stft front end")
    assert worst < TOL_E2E
    assert rel_l2(dx_on, dx_off) < TOL_E2E and rel_l2(w_on, w_off) < TOL_E2E


def test_descript_discriminator_with_the_flag(dev, golden_dir):
    from rave_amd import descript_discriminator as DD
    from test_gpu_parity import TOL_E2E
    g = torch.load(os.path.join(golden_dir, "disc2d_tiny.pt"), weights_only=False)["descript"]
    c = g["config"]
    on, off = (DD.DescriptDiscriminator(periods=c["periods"], fft_sizes=c["fft_sizes"], n_channels=c["n_channels"], hip_frontend=h)
               for h in (True, False))
    sd = g.get("state_dict")
    if sd is None:
        import rave_oracle as O
        sd = O.seeded_state_dict(g["shapes"], g["seed"])
    for m in (on, off):
        m.load_state_dict(sd, strict=False)
        m.to(dev)
    (dx_on, feats), (dx_off, _) = _grads_match(on, off, g["x"].to(dev), lambda m, x: m(x))
    worst = max(rel_l2(f, gf) for net, gnet in zip(feats, g["features"]) for f, gf in zip(net, gnet))
    n_mpd = len(c["periods"])
    first = f"discriminators.{n_mpd}.band_convs.0.0.0.weight_v"
    w_on, w_off = dict(on.named_parameters())[first].grad, dict(off.named_parameters())[first].grad
    print(f"descript, hip_frontend: features {worst:.2e} of the fixture; dx {rel_l2(dx_on, dx_off):.2e}, d {first} {rel_l2(w_on, w_off):.2e} "
          "of the framing kernel + rocFFT front end")
    assert worst < TOL_E2E
    assert rel_l2(dx_on, dx_off) < TOL_E2E and rel_l2(w_on, w_off) < TOL_E2E


def test_recorded_hinge_step_equals_the_eager_one(dev):
    """One discriminator (hinge) step of the shrunk discrete model with the flag on, recorded by GraphedTrainingStep and replayed
    once, against the eager step from the same state: the losses and every discriminator parameter, bit for bit.  (The
    codebooks' running averages go through torch's index_add_ atomics and are no part of what this step trains.)"""
    from rave_amd import model as M
    torch.manual_seed(0)
    m = M.build_discrete(capacity=16, latent_size=16, disc_capacity=16, spectral_capacity=8, num_quantizers=2, codebook_size=32,
                         noise_augmentation=4, update_discriminator_every=2, hip_frontend=True).to(dev).train()
    m.encoder.enabled.fill_(1)
    m.configure_optimizers(capturable=True)
    m.warmed_up = True
    xs = [0.1 * R.white_noise((2, 1, 32768), 90 + i).to(dev) for i in range(3)]
    with torch.no_grad():
        lz = m.encode(xs[0][:1]).shape[-1]
    gen = torch.Generator().manual_seed(6)
    ns = [torch.randn(2, 4, lz, generator=gen).to(dev) for _ in range(3)]
    pre = torch.cuda.Stream()
    pre.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(pre):
        for i in range(2):                               # one eager step of each kind: every codebook and host cache initialised
            m.training_step(xs[i].clone(), i, eps=ns[i], capture_safe=True)
            m.on_train_batch_end(None, None, i)
    torch.cuda.current_stream().wait_stream(pre)
    torch.cuda.synchronize()
    snap = ({k: v.clone() for k, v in m.state_dict().items()}, [M._clone_opt(o) for o in m.optimizers()], m.lr_schedulers().t,
            [[g["lr"].clone() for g in o.param_groups] for o in m.optimizers()])

    def result(logged):
        torch.cuda.synchronize()
        out = {k: v.detach().clone() for k, v in m.discriminator.named_parameters()}
        out.update({"logged." + k: torch.as_tensor(v).detach().clone() for k, v in logged.items()})
        return out

    step = M.GraphedTrainingStep(m, xs[0], inject_eps=True)
    step.eps = torch.zeros_like(ns[0])
    pg = result(step(xs[2], 2, eps=ns[2]))               # step 2 is a discriminator step: recorded, then replayed once
    assert len(step.graphs) == 1
    m.load_state_dict(snap[0])
    for o, st, lrs in zip(m.optimizers(), snap[1], snap[3]):
        M._restore_opt(o, st)
        o.zero_grad(set_to_none=True)
        for gr, lr in zip(o.param_groups, lrs):
            gr["lr"].copy_(lr)
    m.lr_schedulers().t = snap[2]
    M._reset_host_shadows(m)
    for mod in m.modules():
        if hasattr(mod, "refresh_host_caches"):
            mod.refresh_host_caches()
    if m._prep is not None:
        for pr in m._prep:
            pr.invalidate()
    pe = result(m.training_step(xs[2].clone(), 2, eps=ns[2], capture_safe=True))
    assert float(pe["logged.loss_dis"]) != 0.0
    moved = sum(1 for k, v in pe.items() if not k.startswith("logged.") and not torch.equal(v, snap[0]["discriminator." + k]))
    assert moved > 10, moved
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
