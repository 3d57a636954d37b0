"""GPU tests of the instantaneous-frequency distance (rave_amd/csrc/inst_freq_loss.hip, ops.multiscale_inst_freq_distance,
losses.WeightedInstantaneousSpectralDistance) against tests/inst_freq_reference.py in float64, with the torch float32
composition on the CPU as the measure of what float32 can do.

Inputs: g = Generator(seed 0); x = 0.3 randn(3, 2048); y = 0.5 x + 0.2 randn(3, 2048); scales (128, 256, 512), normalized.
These are the smallest shapes with interior, left-edge and right-edge workgroups, more than one span per row at scale 128 and
the frames - 2 edge; "wide" is rows = 1, T = 1025 at scale 2048 (3 frames, all reaching over both reflected ends, one backward
workgroup per row; T = 1024 cannot be reflect-padded by 1024 samples, neither by torch.stft nor by the reference); "silent"
has row 1 of both signals zeroed.

A *flip* is an IF element that differs from the f64 value by ~ 2 pi; on interior bins it may only happen where the f64 value
lies within 1e-3 of +-pi, on bins 0 and n/2 never (there the values are exactly 0 or -pi)."""
import math
from functools import partial

import pytest
import torch

import inst_freq_reference as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

W_UP = (1.0, 0.37)
PI32 = float(torch.tensor(math.pi, dtype=torch.float32))


def _inputs(kind):
    g = torch.Generator().manual_seed(0)
    x = 0.3 * torch.randn(3, 2048, generator=g)
    y = 0.5 * x + 0.2 * torch.randn(3, 2048, generator=g)
    if kind == "wide":
        return x[:1, :1025].contiguous(), y[:1, :1025].contiguous(), (2048,)
    if kind == "silent":
        x[1] = 0
        y[1] = 0
    return x, y, (128, 256, 512)


def _composition(x, y, scales, weighted, dtype):
    x = x.to(dtype).detach().clone().requires_grad_(True)
    y = y.to(dtype).detach().clone().requires_grad_(True)
    sd, pd, ifs = R.distance(x, y, scales, True, weighted, dtype)
    (W_UP[0] * sd + W_UP[1] * pd).backward()
    return dict(sd=float(sd), pd=float(pd), ifs=ifs, gx=x.grad, gy=y.grad)


_REF = {}


def _ref(kind, weighted, dtype):
    """f64 / f32 restatement on the CPU, computed once per case and never modified."""
    key = (kind, weighted, dtype)
    if key not in _REF:
        x, y, scales = _inputs(kind)
        _REF[key] = _composition(x, y, scales, weighted, dtype)
    return _REF[key]


def _windows(scales, dev):
    from rave_amd import losses
    return losses.MultiScaleSTFT(scales, 44100, magnitude=False, normalized=True).to(dev).windows()


def _kernel(kind, weighted, dev, need=(True, True), debug=False, up=W_UP, scales=None):
    from rave_amd import ops
    x, y, sc = _inputs(kind)
    scales = scales or sc
    x = x.to(dev).requires_grad_(need[0])
    y = y.to(dev).requires_grad_(need[1])
    out = ops.multiscale_inst_freq_distance(x, y, _windows(scales, dev), scales, weighted, debug_if=debug)
    (up[0] * out[0] + up[1] * out[1]).backward()
    torch.cuda.synchronize()
    return dict(sd=out[0].detach().cpu(), pd=out[1].detach().cpu(), ifs=out[2] if debug else None,
                gx=None if x.grad is None else x.grad.cpu(), gy=None if y.grad is None else y.grad.cpu())


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _flip_stats(got, want64):
    """(flips, worst non-flip error) of an IF tensor against the f64 one, compared modulo 2 pi."""
    d = got.double() - want64
    flips = d.abs() > math.pi
    dm = torch.remainder(d + math.pi, 2 * math.pi) - math.pi
    return flips, float(dm[~flips].abs().max())


def _if_check(kind, dev, strict=True):
    """Returns the number of flips per scale (all of them allowed ones); ``strict``: with the bound on the worst non-flip error."""
    r64, r32 = _ref(kind, False, torch.float64), _ref(kind, False, torch.float32)
    k = _kernel(kind, False, dev, debug=True)
    counts = []
    for n, (fx64, fy64), (fx32, fy32), ko in zip(_inputs(kind)[2], r64["ifs"], r32["ifs"], k["ifs"]):
        ko = ko.cpu()
        for name, w64, w32, got in (("x", fx64, fx32, ko[:, 0]), ("y", fy64, fy32, ko[:, 1])):
            assert got.shape == w64.shape, (n, got.shape, w64.shape)
            edge = [0, n // 2]
            inner = slice(1, n // 2)
            # the f64 reference alone: how many interior elements sit within 1e-3 of +-pi
            near = (w64[:, inner].abs() - math.pi).abs() < 1e-3
            assert int(near.sum()) <= 1e-3 * near.numel(), \
                f"bad seed: {int(near.sum())} of {near.numel()} f64 IF elements lie within 1e-3 of +-pi (scale {n}, {name})"
            # bins 0 and n/2: exact, in {0, -pi}
            we, ge = w64[:, edge], got[:, edge]
            assert bool(((we.abs() < 1e-9) | ((we + math.pi).abs() < 1e-9)).all()), (n, name)
            assert bool(((ge == 0) | (ge == -PI32)).all()), (n, name)
            assert torch.equal(ge, torch.where(we < -1.0, torch.tensor(-PI32), torch.tensor(0.0)).float()), (n, name)
            # interior bins: flips only next to the wrap boundary, everything else within 4 x the f32 composition's error
            flips, worst = _flip_stats(got[:, inner], w64[:, inner])
            assert bool(near[flips].all()), f"{int((flips & ~near).sum())} flips away from the wrap boundary (scale {n}, {name})"
            tflips, tworst = _flip_stats(w32[:, inner], w64[:, inner])
            print(f"IF {kind} scale {n} {name}: kernel worst {worst:.3e} flips {int(flips.sum())}; torch f32 worst {tworst:.3e} "
                  f"flips {int(tflips.sum())}; {int(near.sum())} of {near.numel()} within 1e-3 of +-pi")
            if worst > 4 * tworst:          # where: the smaller of the two magnitudes behind the worst element, and torch's error there
                sig = _inputs(kind)[0 if name == "x" else 1].double()
                mag = R.stft(sig, n, True).abs()[:, inner]
                low = torch.minimum(mag[..., 2:], mag[..., 1:-1]) / mag.pow(2).mean().sqrt()
                dk = (torch.remainder(got[:, inner].double() - w64[:, inner] + math.pi, 2 * math.pi) - math.pi).abs()
                dt = (torch.remainder(w32[:, inner].double() - w64[:, inner] + math.pi, 2 * math.pi) - math.pi).abs()
                i = int(dk.masked_fill(flips, 0).argmax())
                print(f"   worst kernel element: |S|/rms {float(low.flatten()[i]):.3e}, torch f32 error there {float(dt.flatten()[i]):.3e}; "
                      f"smallest |S|/rms of the tensor {float(low.min()):.3e}; median error kernel {float(dk.median()):.3e} "
                      f"torch {float(dt.median()):.3e}; 99.9 % kernel {float(dk.flatten().kthvalue(int(0.999 * dk.numel())).values):.3e} "
                      f"torch {float(dt.flatten().kthvalue(int(0.999 * dt.numel())).values):.3e}")
            assert not strict or worst <= 4 * tworst, (n, name, worst, tworst)
            counts.append((n, int(flips.sum()), flips.numel() + 2 * flips.shape[0] * flips.shape[2]))
    return counts


@pytest.mark.parametrize("kind", ["main", "wide", "silent"])
def test_inst_freq_elementwise_vs_f64(kind, dev):
    """Measured on an MI355X (profiles/inst_freq_distance.txt): no flips anywhere, the worst element of every tensor within
    0.5 ... 1.8 x the torch f32 composition's.  This is the check that made the kernel transform in f64: with the f32 pair
    transform "main", scale 512, y was 17 x off at the one bin with |S| / rms 4.85e-4."""
    _if_check(kind, dev)
    if kind == "silent":
        k = _kernel(kind, False, dev, debug=True)
        for ko in k["ifs"]:
            assert bool((ko[1] == 0).all())                    # a silent row: phase 0, IF 0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["main", "wide", "silent"])
def test_scalars_and_gradients_vs_f64(kind, weighted, dev):
    """spectral_distance at the 2e-6 of tests/test_gpu_stft_loss.py; phase_distance within 4 x the f32 composition's relative
    error (floor 1e-6) plus (2 pi)^2 flips / numel per counted flip; both gradients, upstream weights (1.0, 0.37), at
    max(1e-4, 4 x the f32 composition's) relative L2.

    Measured on an MI355X (profiles/inst_freq_distance.txt): every gradient at 0.4 ... 1.0 x the f32 composition's error."""
    r64, r32 = _ref(kind, weighted, torch.float64), _ref(kind, weighted, torch.float32)
    k = _kernel(kind, weighted, dev)
    counts = _if_check(kind, dev, strict=False)
    assert abs(float(k["sd"]) - r64["sd"]) <= 2e-6 * abs(r64["sd"]), (float(k["sd"]), r64["sd"])
    flip_part = sum((2 * math.pi) ** 2 * f / numel for _, f, numel in counts) / abs(r64["pd"])
    e32 = abs(r32["pd"] - r64["pd"]) / abs(r64["pd"])
    err = abs(float(k["pd"]) - r64["pd"]) / abs(r64["pd"])
    print(f"{kind} weighted={weighted}: phase_distance rel err kernel {err:.3e}, torch f32 {e32:.3e}; spectral "
          f"{abs(float(k['sd']) - r64['sd']) / abs(r64['sd']):.3e}")
    assert err <= max(1e-6, 4 * e32) + flip_part, (err, e32, flip_part)
    n_flips = sum(f for _, f, _ in counts)
    if n_flips:
        pytest.skip(f"{n_flips} IF elements flipped next to the wrap boundary: gradients not compared")
    for name in ("gx", "gy"):
        e, t = rel_l2(k[name], r64[name]), rel_l2(r32[name], r64[name])
        print(f"   {name}: rel L2 kernel {e:.3e}, torch f32 {t:.3e}")
        assert bool(torch.isfinite(k[name]).all())
        assert e <= max(1e-4, 4 * t), (name, e, t)


def test_silent_row_has_an_exactly_zero_phase_gradient(dev):
    for weighted in (False, True):
        k = _kernel("silent", weighted, dev, up=(0.0, 1.0))
        assert bool((k["gy"][1] == 0).all()) and bool((k["gx"][1] == 0).all())
        assert bool(torch.isfinite(k["gx"]).all()) and bool(torch.isfinite(k["gy"]).all())
        assert float(k["gy"][0].abs().max()) > 0


def test_reproducible_bits_single_gradients_and_accumulation(dev):
    a = _kernel("main", True, dev)
    b = _kernel("main", True, dev)
    for key in ("sd", "pd", "gx", "gy"):
        assert torch.equal(a[key], b[key]), key
    only_y = _kernel("main", True, dev, need=(False, True))
    only_x = _kernel("main", True, dev, need=(True, False))
    assert only_y["gx"] is None and torch.equal(only_y["gy"], a["gy"])
    assert only_x["gy"] is None and torch.equal(only_x["gx"], a["gx"])
    # the scales of one node accumulate in place: the same bits as the separate results added up
    two = _kernel("main", True, dev, scales=(128, 256))
    s128, s256 = _kernel("main", True, dev, scales=(128,)), _kernel("main", True, dev, scales=(256,))
    for key in ("gx", "gy"):
        assert torch.equal(two[key], s128[key] + s256[key]), key


def test_graph_capture_replays_with_eager_bits(dev):
    from rave_amd import ops
    x, y, scales = _inputs("main")
    ws = _windows(scales, dev)
    eager = _kernel("main", True, dev)
    xs, ys = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)

    def step():
        sd, pd = ops.multiscale_inst_freq_distance(xs, ys, ws, scales, True)
        gx, gy = torch.autograd.grad(W_UP[0] * sd + W_UP[1] * pd, (xs, ys))
        return sd, pd, gx, gy

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, key in zip(outs, ("sd", "pd", "gx", "gy")):
            assert torch.equal(got.detach().cpu(), eager[key]), key


def _module(weighted, scales=(128, 256, 512)):
    from rave_amd import losses
    return losses.WeightedInstantaneousSpectralDistance(
        partial(losses.MultiScaleSTFT, scales=list(scales), sample_rate=44100, magnitude=False, normalized=True), weighted=weighted)


def test_module_equals_the_ops_call_and_the_switch_gives_the_composition(dev, monkeypatch):
    from rave_amd import ops
    x, y, scales = _inputs("main")
    k = _kernel("main", True, dev)
    r64, r32 = _ref("main", True, torch.float64), _ref("main", True, torch.float32)

    def run():
        xs, ys = x.to(dev).reshape(3, 1, -1).requires_grad_(True), y.to(dev).reshape(3, 1, -1).requires_grad_(True)
        out = _module(True).to(dev)(xs, ys)
        assert set(out) == {"spectral_distance", "phase_distance"}
        (W_UP[0] * out["spectral_distance"] + W_UP[1] * out["phase_distance"]).backward()
        return out["spectral_distance"].detach().cpu(), out["phase_distance"].detach().cpu(), xs.grad.cpu()[:, 0], ys.grad.cpu()[:, 0]

    sd, pd, gx, gy = run()
    assert torch.equal(sd, k["sd"]) and torch.equal(pd, k["pd"]) and torch.equal(gx, k["gx"]) and torch.equal(gy, k["gy"])
    monkeypatch.setenv("RH_INST_FREQ", "0")
    monkeypatch.setattr(ops, "multiscale_inst_freq_distance", lambda *a, **kw: pytest.fail("RH_INST_FREQ=0 ran the kernels"))
    sd, pd, gx, gy = run()
    assert abs(float(sd) - r64["sd"]) <= 2e-6 * abs(r64["sd"])
    assert abs(float(pd) - r64["pd"]) / abs(r64["pd"]) <= max(1e-6, 4 * abs(r32["pd"] - r64["pd"]) / abs(r64["pd"]))
    for got, name in ((gx, "gx"), (gy, "gy")):
        assert rel_l2(got, r64[name]) <= max(1e-4, 4 * rel_l2(r32[name], r64[name])), name


def test_training_step_with_the_phase_distance(dev):
    """build_v2(phase_distance=True) at the tiny width: one VAE-phase step logs fullband_phase_distance and every generator
    parameter receives a finite gradient."""
    import rave_oracle as O
    from rave_amd import losses, model as M
    torch.manual_seed(0)
    m = M.build_v2(phase_distance=True, capacity=16, latent_size=16, disc_capacity=16).to(dev).train()
    assert isinstance(m.audio_distance, losses.WeightedInstantaneousSpectralDistance) and m.audio_distance.weighted
    assert isinstance(m.multiband_audio_distance, losses.AudioDistanceV1)
    m.configure_optimizers()
    x = O.synthetic_batch(2, 1, 32768).to(dev)
    eps = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(0)).to(dev)
    grads = {}
    hooks = [p.register_hook(lambda g, n=n: grads.__setitem__(n, g.detach().clone())) for n, p in m.named_parameters() if p.requires_grad]
    logged = m.training_step(x, 0, eps=eps)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert "fullband_phase_distance" in logged and "fullband_spectral_distance" in logged
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logged.values())
    want = [n for n, p in m.named_parameters() if p.requires_grad and n.startswith(("encoder.", "decoder."))]
    assert want and all(n in grads for n in want), [n for n in want if n not in grads]
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), n
