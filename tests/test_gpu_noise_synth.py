"""The filtered-noise synthesis kernels (csrc/noise_synth.hip) and the noise generators on them, against the float64 torch
composition (tests/noise_synth_reference.py): values and gradients at every shipped size and at the edges of the built range,
run-to-run identity, 4-byte aligned pointers, the modules on both paths, an unbuilt size, and a recorded graph."""
import functools

import pytest
import torch

import noise_synth_reference as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-4                     # the project's bound on relative L2 against float64

# v1.gin, v2_small.gin (filter cropped), noise.gin, the smallest, the largest, an odd target size with a cropped filter
SIZES = [(5, 64), (32, 8), (5, 8), (2, 4), (33, 64), (5, 3)]
# (channels, frames): a single item; fewer frames and channels than a tile; several tiles with a ragged last one in t
EXTENTS = [(1, 1), (3, 5), (16, 67)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(nb, n, d, t):
    """float64 inputs and the composition's (out, gh) for them, computed once per size."""
    h, noise, gout = R.inputs(nb, n, d, t)
    out, gh = R.composition_with_grad(h, noise, gout, nb, n)
    return h, noise, gout, out, gh


def _run(h, noise, gout, nb, n, dev):
    from rave_amd import ops
    table = ops.noise_synth_table(nb, n).to(dev)
    hg = h.float().to(dev).requires_grad_(True)
    out = ops.noise_synth(hg, noise.float().to(dev), table, nb, n)
    (gh,) = torch.autograd.grad(out, hg, gout.float().to(dev))
    return out.detach(), gh


@pytest.mark.parametrize("d,t", EXTENTS)
@pytest.mark.parametrize("nb,n", SIZES)
def test_forward_and_backward_against_float64(dev, nb, n, d, t):
    h, noise, gout, want, want_gh = _case(nb, n, d, t)
    out, gh = _run(h, noise, gout, nb, n, dev)
    assert tuple(out.shape) == (2, d, t * n) and tuple(gh.shape) == tuple(h.shape)
    c_out, c_gh = R.composition_with_grad(h.float().to(dev), noise.float().to(dev), gout.float().to(dev), nb, n)
    print(f"noise_synth nb={nb} N={n} D={d} T={t}: out rel L2 {rel_l2(out, want):.2e} (f32 composition {rel_l2(c_out, want):.2e}), "
          f"gh rel L2 {rel_l2(gh, want_gh):.2e} (f32 composition {rel_l2(c_gh, want_gh):.2e})")
    assert rel_l2(out, want) <= TOL
    assert rel_l2(gh, want_gh) <= TOL
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gh).all())


@pytest.mark.parametrize("nb,n", [(5, 64), (32, 8)])
def test_two_runs_give_the_same_bits(dev, nb, n):
    h, noise, gout, _, _ = _case(nb, n, 16, 67)
    a, b = _run(h, noise, gout, nb, n, dev), _run(h, noise, gout, nb, n, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("nb,n", [(5, 64), (32, 8), (5, 3)])
def test_pointers_that_are_only_4_byte_aligned(dev, nb, n):
    """Every operand one float past a 16-byte boundary (and at the other residues), inside guard bands: the same bits as the
    aligned call, and nothing written outside the outputs."""
    import misaligned as MA
    from rave_amd import _lib as L
    from rave_amd import ops
    d, t = 3, 5
    h64, noise64, gout64, _, _ = _case(nb, n, d, t)
    h, noise, gout = (v.float().to(dev) for v in (h64, noise64, gout64))
    table = ops.noise_synth_table(nb, n).to(dev)

    def fwd(h_, noise_, table_, out_):
        return L.lib.rh_noise_synth_fwd_f32(L.ptr(h_), L.ptr(noise_), L.ptr(table_), 2, d, t, nb, n, L.ptr(out_), L.stream())

    def bwd(h_, noise_, table_, gout_, gh_):
        return L.lib.rh_noise_synth_bwd_f32(L.ptr(h_), L.ptr(noise_), L.ptr(table_), L.ptr(gout_), 2, d, t, nb, n, L.ptr(gh_),
                                            L.stream())

    base_out, base_gh = torch.zeros_like(gout), torch.zeros_like(h)
    assert all(v.data_ptr() % 256 == 0 for v in (h, noise, gout, table, base_out, base_gh))
    assert fwd(h, noise, table, base_out) == 0 and bwd(h, noise, table, gout, base_gh) == 0
    for off in (1, 2, 3):
        hs, ns, gs, ts = MA.carve(h, off), MA.carve(noise, off), MA.carve(gout, off), MA.carve(table, off)
        outs, ghs = MA.carve(torch.zeros_like(gout), off), MA.carve(torch.zeros_like(h), off)
        assert fwd(hs, ns, ts, outs) == 0 and bwd(hs, ns, ts, gs, ghs) == 0
        torch.cuda.synchronize()
        assert torch.equal(outs, base_out) and torch.equal(ghs, base_gh), off
        assert all(MA.guards_intact(v) for v in (hs, ns, gs, ts, outs, ghs)), off
    assert float(base_out.abs().max()) > 0 and float(base_gh.abs().max()) > 0


def _modules(dev):
    from rave_amd import blocks
    torch.manual_seed(11)
    v1 = blocks.NoiseGenerator(in_size=8, data_size=4).to(dev)
    v2 = blocks.NoiseGeneratorV2(8, 16, 4, [2, 2, 2], 5, n_channels=2).to(dev)
    gen = torch.Generator().manual_seed(12)
    # (module, input, shape of the draw (B, T, D, N)): 128 / 64 samples in, T = 2 / 8 frames
    return [(v1, torch.randn(2, 8, 128, generator=gen).to(dev), (2, 2, 4, 64)),
            (v2, torch.randn(2, 8, 64, generator=gen).to(dev), (2, 8, 8, 8))]


def _module_pass(m, x, noise, cot, seed=None):
    """Output and every parameter gradient of one forward + backward pass."""
    from rave_amd import ops
    ops.range_reset(x.device)
    if seed is not None:
        torch.manual_seed(seed)
    out = m(x, noise=noise)
    params = list(m.parameters())
    grads = torch.autograd.grad(out, params, cot)
    ops.join_side_streams()
    return [out.detach()] + list(grads)


def test_modules_on_the_kernel_and_on_the_composition(dev, monkeypatch):
    """NoiseGenerator and NoiseGeneratorV2: the kernel path against the RH_NOISE_SYNTH=0 path, output and all parameter
    gradients, with injected noise and -- under one seed -- with the modules' own draw (both paths see the same stream)."""
    from rave_amd import ops
    calls = []
    real = ops.noise_synth
    monkeypatch.setattr(ops, "noise_synth", lambda *a: (calls.append(1), real(*a))[1])
    for m, x, shape in _modules(dev):
        gen = torch.Generator().manual_seed(13)
        noise = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        cot = torch.randn(shape[0], shape[2], shape[1] * shape[3], generator=gen).to(dev)
        for injected, seed in ((noise, None), (None, 14)):
            monkeypatch.setenv("RH_NOISE_SYNTH", "1")
            got = _module_pass(m, x, injected, cot, seed)
            assert len(calls) == 1
            monkeypatch.setenv("RH_NOISE_SYNTH", "0")
            want = _module_pass(m, x, injected, cot, seed)
            assert len(calls) == 1                                  # the switch took the composition
            calls.clear()
            for a, b in zip(got, want):
                assert float(b.abs().max()) > 0
                assert rel_l2(a, b) <= TOL, (type(m).__name__, seed, tuple(a.shape), rel_l2(a, b))


def test_unbuilt_size_runs_the_composition(dev):
    """noise_bands = 40 is outside the built range: no table, the torch composition on the GPU, right against float64."""
    from rave_amd import blocks, ops
    torch.manual_seed(15)
    m = blocks.NoiseGeneratorV2(8, 16, 2, [2, 2, 2], 40).to(dev)
    assert m.noise_table is None and not ops.noise_synth_supported(40, 8)
    x = torch.randn(2, 8, 32).to(dev)
    noise = (torch.rand(2, 4, 2, 8) * 2 - 1).to(dev)
    hooked = []
    handle = m.net[-1].register_forward_hook(lambda mod, args, out: hooked.append(out.detach()))
    ops.range_reset(dev)
    out = m(x, noise=noise)
    handle.remove()
    want = R.composition(hooked[0].double().cpu(), noise.double().cpu(), 40, 8)
    assert tuple(out.shape) == (2, 2, 32) and rel_l2(out, want) <= TOL


def test_recorded_pass_equals_the_eager_one(dev):
    """Forward + backward of NoiseGeneratorV2 recorded into a graph (on the capture's own, non-default stream) after one warm
    eager call, replayed twice: the bits of the eager call."""
    from rave_amd import ops
    _, (m, x, shape) = _modules(dev)
    gen = torch.Generator().manual_seed(16)
    noise = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
    cot = torch.randn(shape[0], shape[2], shape[1] * shape[3], generator=gen).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [v.clone() for v in _module_pass(m, x, noise, cot)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        recorded = _module_pass(m, x, noise, cot)
    pools = ops.range_capture_end()                                  # the graph's range slots live as long as it does
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(recorded, eager):
            assert torch.equal(a, b)
    assert float(eager[0].abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in eager[1:])
    del graph, pools
