"""The recurrent latent layer on the GPU (rave_amd/csrc/gru.hip, ops.gru, blocks.GRU; rave/blocks.py:295-319) against
``torch.nn.GRU`` in float64 on the CPU with the same weights, between the reference's two permutes.

Bar: relative L2 <= 1e-4 (the project's parity bar), separately for the output, dx and every parameter gradient.  The
reference's own float32 module on the CPU sits at <= 1e-6 from float64 on these inputs.  Measured on the MI355X
(profiles/gru.txt): output <= 4.1e-7, dx <= 9.4e-7, parameter gradients <= 9.4e-7 over all shapes and modes below."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rave_oracle as O  # noqa: E402  (input batches only)

pytestmark = pytest.mark.gpu

BAR = 1e-4
#         B, H,   T,  L
SHAPES = [(1, 16, 1, 1),       # no recurrence at all, h0 = 0
          (2, 16, 2, 1),       # the first real step
          (3, 48, 7, 2),       # H not a power of two, odd B and T; also the fixture's shape
          (1, 128, 37, 2),     # largest H: the register-resident weights full
          (5, 128, 3, 3),
          (2, 64, 33, 4)]
PARAM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def make_case(shape, w_scale=1.0, x_scale=1.0, seed=0):
    """Default-initialised weights (times w_scale) and an input whose values differ along every axis."""
    from rave_amd import blocks
    b, h, t, n_layers = shape
    torch.manual_seed(100 + seed)
    m = blocks.GRU(h, n_layers)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(w_scale)
    gen = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(b, h, t, generator=gen) * x_scale
    dy = torch.randn(b, h, t, generator=gen)
    return m, x, dy


_REF = {}


def reference(m, x, dy, key):
    """torch.nn.GRU in float64 on the CPU: output, dx and parameter gradients (computed once per case)."""
    if key not in _REF:
        n_layers = m.num_layers
        h = x.shape[1]
        ref = torch.nn.GRU(input_size=h, hidden_size=h, num_layers=n_layers, batch_first=True).double()
        ref.load_state_dict({k[len("gru."):]: v.double() for k, v in m.state_dict().items() if k.startswith("gru.")})
        xr = x.double().clone().requires_grad_(True)
        y = ref(xr.permute(0, 2, 1))[0].permute(0, 2, 1)
        y.backward(dy.double())
        _REF[key] = (y.detach(), xr.grad, {n: p.grad for n, p in ref.named_parameters()})
    return _REF[key]


def run_module(m, x, dy, dev):
    m = m.to(dev)
    for p in m.parameters():
        p.grad = None
    xg = x.to(dev).requires_grad_(True)
    y = m(xg)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    return y.detach(), xg.grad, {n: p.grad for n, p in m.gru.named_parameters()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_under_no_grad(dev, shape):
    m, x, dy = make_case(shape)
    y_ref = reference(m, x, dy, (shape, 1.0, 1.0))[0]
    m = m.to(dev)
    with torch.no_grad():
        y = m(x.to(dev))
    e = rel(y, y_ref)
    print(f"gru no_grad {shape}: y {e:.2e}")
    assert y.shape == x.shape and not y.requires_grad
    assert e <= BAR


@pytest.mark.parametrize("scales", [(1.0, 1.0), (3.0, 2.0)], ids=["default", "w3x2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_backward(dev, shape, scales):
    m, x, dy = make_case(shape, *scales)
    y_ref, dx_ref, g_ref = reference(m, x, dy, (shape,) + scales)
    y, dx, g = run_module(m, x, dy, dev)
    errs = {"y": rel(y, y_ref), "dx": rel(dx, dx_ref)}
    for n in g_ref:
        errs[n] = rel(g[n], g_ref[n])
    print(f"gru fwd+bwd {shape} w x{scales[0]} x x{scales[1]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(g) == set(g_ref)
    for k, v in errs.items():
        assert v <= BAR, (k, v)


def test_fixture_of_the_reference_module(dev, golden_dir):
    """The recorded run of the unmodified rave.blocks.GRU (float32, CPU): its checkpoint loads, and output and gradients agree."""
    from rave_amd import blocks
    fx = torch.load(os.path.join(golden_dir, "gru_tiny.pt"), weights_only=False)
    b, h, t, n_layers = fx["shape"]
    assert (b, h, t, n_layers) == (3, 48, 7, 2)
    m = blocks.GRU(h, n_layers)
    m.load_state_dict(fx["state_dict"], strict=True)
    y, dx, g = run_module(m, fx["x"], fx["dy"], dev)
    assert rel(y, fx["y"]) <= BAR and rel(dx, fx["dx"]) <= BAR
    assert set(fx["grads"]) == {"gru." + n for n in g}
    for n, v in g.items():
        assert rel(v, fx["grads"]["gru." + n]) <= BAR, n


def test_saturated_gates_stay_finite(dev):
    shape = (2, 48, 9, 2)
    m, x, dy = make_case(shape, w_scale=3.0)
    x = torch.where(x > 0, torch.full_like(x, 50.0), torch.full_like(x, -50.0))
    y, dx, g = run_module(m, x, dy, dev)
    y_ref, dx_ref, g_ref = reference(m, x, dy, "saturated")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    assert float(y.abs().max()) <= 1.0
    assert rel(y, y_ref) <= BAR


def test_same_call_twice_is_bit_identical(dev):
    shape = (5, 128, 3, 3)
    m, x, dy = make_case(shape, 3.0, 2.0)
    y1, dx1, g1 = run_module(m, x, dy, dev)
    y1, dx1, g1 = y1.clone(), dx1.clone(), {n: v.clone() for n, v in g1.items()}
    y2, dx2, g2 = run_module(m, x, dy, dev)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


def test_layout_time_is_the_innermost_axis(dev):
    """An input that differs along every axis and is NOT symmetric under swapping H and T (H == T here on purpose, so that a
    kernel reading (B, T, H) runs without a shape error and must fail on the values)."""
    shape = (2, 16, 16, 1)
    m, x, dy = make_case(shape)
    b_i, h_i, t_i = torch.meshgrid(torch.arange(2.), torch.arange(16.), torch.arange(16.), indexing="ij")
    x = 0.3 * torch.sin(0.9 * h_i + 0.1) + 0.05 * t_i - 0.4 * b_i + 0.02 * h_i * t_i * (b_i + 1)
    assert not torch.equal(x, x.transpose(1, 2)) and len(x.unique()) > 400
    y_ref, dx_ref, _ = reference(m, x, dy, "layout")
    y_swapped = reference(m, x.transpose(1, 2).contiguous(), dy, "layout-swapped")[0].transpose(1, 2)
    assert rel(y_swapped, y_ref) > 1e-2                  # the wrong reading is far outside the bar
    y, dx, _ = run_module(m, x, dy, dev)
    assert rel(y, y_ref) <= BAR and rel(dx, dx_ref) <= BAR


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "one-float-past-16B"])
def test_c_abi_inside_guarded_buffers(dev, misalign):
    """Every buffer of both entry points inside a guarded allocation (tests/misaligned.py: NaN guards, so an out-of-bounds
    READ poisons the result and an out-of-bounds WRITE is seen bit for bit); in the second case x, one weight and the output
    start one float past a 16-byte boundary."""
    from misaligned import carve, guards_intact
    from rave_amd import _lib as L
    shape = (3, 48, 7, 2)
    b, h, t, n_layers = shape
    m, x, dy = make_case(shape, 3.0, 2.0)
    y_ref, dx_ref, g_ref = reference(m, x, dy, (shape, 3.0, 2.0))
    off = 1 if misalign else 0
    params = {n: carve(p.detach().to(dev), off if n == "weight_hh_l1" else 0) for n, p in m.gru.named_parameters()}
    grads = {n: carve(torch.zeros_like(p), 0) for n, p in params.items()}
    xg, dyg = carve(x.to(dev), off), carve(dy.to(dev), 0)
    y, dx = carve(torch.zeros(b, h, t, device=dev), off), carve(torch.zeros(b, h, t, device=dev), 0)
    if misalign:
        assert xg.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 4 and params["weight_hh_l1"].data_ptr() % 16 == 4
    nbytes = C.c_int64(0)
    L.check(L.lib.rh_gru_workspace_bytes(b, h, t, n_layers, 1, C.byref(nbytes)), "gru_workspace_bytes")
    ws = carve(torch.zeros(nbytes.value // 4, device=dev), off)
    items = (L.GruItem * n_layers)()
    for k in range(n_layers):
        for f in PARAM_NAMES:
            setattr(items[k], f.replace("weight", "w").replace("bias", "b"), params[f"{f}_l{k}"].data_ptr())
            setattr(items[k], "d" + f.replace("weight", "w").replace("bias", "b"), grads[f"{f}_l{k}"].data_ptr())
    L.check(L.lib.rh_gru_fwd_f32(xg.data_ptr(), items, n_layers, b, h, t, 1, y.data_ptr(), ws.data_ptr(), nbytes.value,
                                 L.stream()), "gru_fwd")
    L.check(L.lib.rh_gru_bwd_f32(dyg.data_ptr(), xg.data_ptr(), items, n_layers, b, h, t, dx.data_ptr(), ws.data_ptr(),
                                 nbytes.value, L.stream()), "gru_bwd")
    torch.cuda.synchronize()
    for name, v in [("x", xg), ("dy", dyg), ("y", y), ("dx", dx), ("ws", ws)] + list(params.items()) + list(grads.items()):
        assert guards_intact(v), name
    assert torch.equal(xg.cpu(), x) and torch.equal(dyg.cpu(), dy)       # inputs are only read
    for n, p in m.gru.named_parameters():
        assert torch.equal(params[n].cpu(), p.detach().cpu()), n
    assert rel(y, y_ref) <= BAR and rel(dx, dx_ref) <= BAR
    for n in g_ref:
        assert rel(grads[n], g_ref[n]) <= BAR, n
    # the inference workspace is smaller and keeps nothing: same output
    L.check(L.lib.rh_gru_workspace_bytes(b, h, t, n_layers, 0, C.byref(nbytes)), "gru_workspace_bytes")
    ws0 = carve(torch.zeros(nbytes.value // 4, device=dev), off)
    y0 = carve(torch.zeros(b, h, t, device=dev), off)
    L.check(L.lib.rh_gru_fwd_f32(xg.data_ptr(), items, n_layers, b, h, t, 0, y0.data_ptr(), ws0.data_ptr(), nbytes.value,
                                 L.stream()), "gru_fwd")
    torch.cuda.synchronize()
    assert guards_intact(ws0) and guards_intact(y0) and torch.equal(y0, y)


def test_disable_is_the_identity_and_enable_restores(dev):
    m, x, _ = make_case((2, 16, 5, 1))
    m = m.to(dev)
    xg = x.to(dev)
    with torch.no_grad():
        y = m(xg)
        m.disable()
        assert m(xg) is xg
        m.enable()
        y2 = m(xg)
    assert y2 is not xg and torch.equal(y, y2) and not torch.equal(y, xg)


# ---- model level: a shrunk v2 with the layer in front of the decoder ------------------------------------------------------

KW = dict(capacity=16, latent_size=16, disc_capacity=16, gru_layers=2)
STEPS = 3


def _train(dev, graphed):
    from rave_amd import model as M
    torch.manual_seed(0)
    m = M.build_v2(**KW).to(dev).train()
    m.configure_optimizers(capturable=True)
    xs = [O.synthetic_batch(2, 1, 32768, seed=70 + i).to(dev) for i in range(STEPS)]
    gen = torch.Generator().manual_seed(2)
    es = [torch.randn(2, 16, 16, generator=gen).to(dev) for _ in range(STEPS)]
    step = M.GraphedTrainingStep(m, xs[0], inject_eps=True) if graphed else None
    for i in range(STEPS):
        if graphed:
            step(xs[i], i, eps=es[i])
        else:
            m.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
        m.on_train_batch_end(None, None, i)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in m.named_parameters()}


def test_vae_phase_step_gives_every_gru_parameter_a_gradient_and_is_repeatable(dev):
    from rave_amd import model as M

    def one():
        torch.manual_seed(0)
        m = M.build_v2(**KW).to(dev).train()
        m.configure_optimizers()
        x = O.synthetic_batch(2, 1, 32768).to(dev)
        eps = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(0)).to(dev)
        grads = {}
        hooks = [p.register_hook(lambda g, n=n: grads.__setitem__(n, g.detach().clone()))
                 for n, p in m.named_parameters() if ".gru." in n]
        logged = m.training_step(x, 0, eps=eps)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        return grads, {k: v.detach().clone() for k, v in m.named_parameters()}, logged

    g1, p1, logged = one()
    assert sorted(g1) == sorted(f"decoder.net.0.gru.{n}_l{k}" for k in range(2) for n in PARAM_NAMES)
    for n, g in g1.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in logged.values())
    g2, p2, _ = one()
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n


def test_graphed_vae_phase_steps_are_bit_identical_to_eager(dev):
    pe = _train(dev, graphed=False)
    pg = _train(dev, graphed=True)
    assert any(".gru." in k for k in pe)
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    from rave_amd import model as M
    torch.manual_seed(0)
    m0 = M.build_v2(**KW)
    for k, v in m0.named_parameters():
        if ".gru." in k:
            assert not torch.equal(v.detach(), pe[k].cpu()), k            # the optimizer moved the recurrent layer
