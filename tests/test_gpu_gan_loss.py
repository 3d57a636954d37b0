"""The GAN-objective kernels (csrc/gan_loss.hip) behind rave_amd.ops.gan_losses, rave_amd.losses' three functions and
RAVE.training_step, against the float64 restatement of tests/gan_loss_reference.py: values and gradients at every size at which
the kernel takes another path (fewer scores than a vector, a ragged last vector, one lane / wave / workgroup more or less), tables
of unequal heads, unsplit / split / permuted feeds, the recorded fixture of the reference, 4-byte aligned pointers, run-to-run
identity, a recorded graph, and the training step on both paths.

Bounds.  Gradients: relative L2 <= 1e-4 against float64.  Scalars: |got - f64| <= max(derived, 2 x the error of the float32 ATen
composition on the same inputs), derived = gan_loss_reference.derived_bound (per head 16 u (1 + mean |summand|), plus the worst
case of the ordered float32 sum over the heads)."""
import functools
import os

import pytest
import torch

import gan_loss_reference as R
from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-4
CHUNK = 4096                    # kGanChunk: scores of one half per workgroup
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1]
GRAD_OUT = (1.0, 0.5)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _table_sizes(count):
    """Unequal halves for a table of ``count`` heads: every size of SIZES in turn, plus sizes of several workgroups."""
    pool = SIZES + [2 * CHUNK + 8, 37, 1000, 3 * CHUNK + 3]
    return tuple(pool[(3 * i + count) % len(pool)] for i in range(count))


@functools.lru_cache(maxsize=None)
def _case(mode, sizes, grad_out=GRAD_OUT):
    """float64 heads and the restatement's totals / gradients for them, computed once per (objective, sizes)."""
    heads = [R.scores(n, 100 + 7 * i + n, mode) for i, n in enumerate(sizes)]
    out, grads, mean_abs, head_means = R.totals(mode, heads, torch.float64, grad_out)
    return heads, out, grads, mean_abs, head_means


def _feed(heads64, how, dev):
    """Device inputs for ops.gan_losses and the leaves whose .grad holds (d_real, d_fake) afterwards."""
    fed, leaves = [], []
    for r, f in heads64:
        r, f = r.float().reshape(-1, 1), f.float().reshape(-1, 1)             # (B, 1): one score per batch row
        if how == "pairs":
            a, b = r.to(dev).requires_grad_(True), f.to(dev).requires_grad_(True)
            fed.append((a, b))
            leaves.append(lambda a=a, b=b: (a.grad, b.grad))
        else:
            t = torch.cat([r, f], 0).to(dev).requires_grad_(True)
            fed.append(t if how == "unsplit" else tuple(torch.split(t, t.shape[0] // 2, 0)))
            leaves.append(lambda t=t: tuple(torch.split(t.grad, t.shape[0] // 2, 0)))
    return fed, leaves


def _check(mode, sizes, how, dev, grad_out=GRAD_OUT):
    from rave_amd import ops
    heads64, want, want_g, mean_abs, head_means = _case(mode, tuple(sizes), grad_out)
    fed, leaves = _feed(heads64, how, dev)
    out = ops.gan_losses(fed, mode)
    assert len(out) == 4 and all(v.dim() == 0 and v.dtype == torch.float32 for v in out)
    assert out[0].requires_grad and out[1].requires_grad and not out[2].requires_grad and not out[3].requires_grad
    torch.autograd.backward([out[0], out[1]], [torch.tensor(g, device=dev) for g in grad_out])
    aten = R.totals(mode, [(r.float().to(dev), f.float().to(dev)) for r, f in heads64], torch.float32, grad_out)[0]
    worst = 0.0
    for k, name in enumerate(("loss_dis", "loss_adv", "pred_real", "pred_fake")):
        err = abs(float(out[k].double().cpu()) - float(want[k]))
        aten_err = abs(float(aten[k].double().cpu()) - float(want[k]))
        bound = max(R.derived_bound(mean_abs, head_means, k), 2 * aten_err)
        print(f"gan_loss {mode} {how} heads={len(sizes)} n={sizes[:4]}: {name} err {err:.3e} (ATen f32 {aten_err:.3e}, "
              f"derived {R.derived_bound(mean_abs, head_means, k):.3e})")
        assert err <= bound, (name, err, bound)
        worst = max(worst, err)
    for (dr, df), (wr, wf), n in zip((leaf() for leaf in leaves), want_g, sizes):
        assert dr.numel() == n and df.numel() == n
        got, ref = torch.cat([dr.reshape(-1), df.reshape(-1)]), torch.cat([wr, wf])
        assert bool(torch.isfinite(got).all())
        assert rel_l2(got, ref) <= TOL, (n, rel_l2(got, ref))
        zero = R.planted(mode, n)
        for k in zero["real"]:
            assert float(dr.reshape(-1)[k]) == 0.0, (n, k)
        for k in zero["fake_all"] + (zero["fake_dis"] if grad_out[1] == 0 else []):
            assert float(df.reshape(-1)[k]) == 0.0, (n, k)
    return worst


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", R.MODES)
def test_one_head_against_float64(dev, mode, n):
    _check(mode, (n,), "pairs", dev)


@pytest.mark.parametrize("how", ["unsplit", "split", "pairs"])
@pytest.mark.parametrize("count", [1, 2, 80])
@pytest.mark.parametrize("mode", R.MODES)
def test_tables_of_unequal_heads_against_float64(dev, mode, count, how):
    _check(mode, _table_sizes(count), how, dev)


@pytest.mark.parametrize("n", [5, 257, CHUNK + 1])
@pytest.mark.parametrize("mode", ["hinge", "nonsaturating"])
def test_closed_gates_give_exact_zeros(dev, mode, n):
    """Hinge: r == 1 and f == -1 exactly (the gates are closed at equality); non-saturating: +-20, outside the clamp.  With
    d / d loss_adv = 0 the fake half is gated as well (adv = -f always passes)."""
    assert R.planted(mode, n)["real"] and R.planted(mode, n)["fake_dis"]
    _check(mode, (n,), "unsplit", dev, grad_out=(1.0, 0.0))
    if mode == "nonsaturating":
        _check(mode, (n,), "unsplit", dev, grad_out=(0.0, 1.0))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
def test_permuted_dense_views_are_used_in_place(dev, mode, split):
    """A period-major (2B, 1, T, p) score map -- a permuted view of a dense (2B, p, T) tensor, what the period discriminators hand
    out --, unsplit and as torch.split views: no copy, and the gradient arrives in the view's own memory order."""
    from rave_amd import ops
    b2, p, t = 4, 3, 35
    g = torch.Generator().manual_seed(40)
    base64 = (2 * torch.randn(b2, p, t, generator=g, dtype=torch.float64)).clamp(-13, 13).float().double()
    leaf = base64.float().to(dev).requires_grad_(True)
    view = leaf.permute(0, 2, 1).unsqueeze(1)
    assert tuple(view.shape) == (b2, 1, t, p) and not view.is_contiguous() and ops._dense_batch_major(view)
    halves = torch.split(view, b2 // 2, 0)
    assert all(ops._dense_any_order(h) and not h.is_contiguous() for h in halves)
    copies = []
    real_contiguous = torch.Tensor.contiguous
    try:
        torch.Tensor.contiguous = lambda self, *a, **k: (copies.append(1), real_contiguous(self, *a, **k))[1]
        out = ops.gan_losses([tuple(halves) if split else view], mode)
    finally:
        torch.Tensor.contiguous = real_contiguous
    assert not copies
    torch.autograd.backward([out[0], out[1]], [torch.tensor(v, device=dev) for v in GRAD_OUT])
    v64 = base64.permute(0, 2, 1).unsqueeze(1)
    heads = [(v64[:b2 // 2].reshape(-1), v64[b2 // 2:].reshape(-1))]
    want, want_g, mean_abs, head_means = R.totals(mode, heads, torch.float64, GRAD_OUT)
    aten = R.totals(mode, [(h[0].float().to(dev), h[1].float().to(dev)) for h in heads], torch.float32, GRAD_OUT)[0]
    for k in range(4):
        err = abs(float(out[k].double().cpu()) - float(want[k]))
        assert err <= max(R.derived_bound(mean_abs, head_means, k), 2 * abs(float(aten[k].double().cpu()) - float(want[k]))), k
    got = leaf.grad.permute(0, 2, 1).unsqueeze(1)                 # the same view of the gradient
    ref = torch.cat([want_g[0][0], want_g[0][1]]).reshape(b2, 1, t, p)
    assert rel_l2(got, ref) <= TOL, rel_l2(got, ref)


@pytest.mark.parametrize("mode", R.MODES)
def test_the_reference_fixture(dev, mode):
    """tests/golden/gan_loss_tiny.pt (the unmodified reference on the CPU, tools/make_golden_gan_loss.py) through
    rave_amd.losses' drop-in functions: the float64 record is the yardstick, the float32 record the ATen composition."""
    from rave_amd import losses
    fx = torch.load(os.path.join(GOLDEN, "gan_loss_tiny.pt"))
    rec = fx[mode]
    g = tuple(fx["grad_out"].tolist())
    r = rec["real"].to(dev).requires_grad_(True)
    f = rec["fake"].to(dev).requires_grad_(True)
    dis, adv = losses.GAN_LOSSES[mode](r, f)
    (g[0] * dis + g[1] * adv).backward()
    d64, a64 = R.terms(mode, rec["real"].double().reshape(-1), rec["fake"].double().reshape(-1))
    for got, key, term in ((dis, "loss_dis", d64), (adv, "loss_adv", a64)):
        want = float(rec["f64"][key])
        bound = max(16 * R.U * (1 + float(term.abs().mean())), 2 * abs(float(rec["f32"][key]) - want))
        assert abs(float(got) - want) <= bound, (key, float(got), want, bound)
    assert r.grad.shape == rec["real"].shape
    assert rel_l2(r.grad, rec["f64"]["d_real"]) <= TOL and rel_l2(f.grad, rec["f64"]["d_fake"]) <= TOL


@pytest.mark.parametrize("mode", ["hinge", "ls"])
def test_unequal_shapes_broadcast_as_in_the_reference(dev, mode, monkeypatch):
    """(2, 1, 9) real against (2, 9, 1) fake scores: equally many, but the reference's dis expression broadcasts them to
    (2, 9, 9) -- the drop-in functions run the composition there, never the kernel."""
    from rave_amd import losses, ops
    monkeypatch.setattr(ops, "gan_losses", lambda *a: pytest.fail("the kernel took scores of unequal shapes"))
    g = torch.Generator().manual_seed(41)
    r, f = torch.randn(2, 1, 9, generator=g).to(dev), torch.randn(2, 9, 1, generator=g).to(dev)
    dis, adv = losses.GAN_LOSSES[mode](r, f)
    want_d, want_a = R.terms(mode, r.double().cpu(), f.double().cpu())
    assert tuple(want_d.shape) == (2, 9, 9)
    for got, want in ((dis, want_d), (adv, want_a)):
        assert abs(float(got) - float(want.mean())) <= 16 * R.U * (1 + float(want.abs().mean()))


def _raw_items(heads, grads=None):
    from rave_amd import _lib as L
    arr = (L.GanItem * len(heads))()
    for i, (a, (r, f)) in enumerate(zip(arr, heads)):
        a.real, a.fake, a.n = r.data_ptr(), f.data_ptr(), r.numel()
        a.d_real, a.d_fake = (None, None) if grads is None else (grads[i][0].data_ptr(), grads[i][1].data_ptr())
    return arr


def _raw_call(mode_id, heads, grads, g, dev):
    """Both entry points on caller-placed buffers; returns (sums, out)."""
    from rave_amd import _lib as L
    n = len(heads)
    arr = _raw_items(heads, grads)
    nbytes = L.lib.rh_gan_loss_workspace_bytes(arr, n)
    assert nbytes == 16 * sum((r.numel() + CHUNK - 1) // CHUNK for r, _ in heads)
    ws = torch.empty(nbytes // 4, device=dev)
    sums, out = torch.zeros(n, 4, device=dev), torch.zeros(4, device=dev)
    assert L.lib.rh_gan_loss_fwd_f32(arr, n, mode_id, L.ptr(ws), nbytes, L.ptr(sums), L.ptr(out), L.stream()) == 0
    assert L.lib.rh_gan_loss_bwd_f32(arr, n, mode_id, L.ptr(g), L.stream()) == 0
    torch.cuda.synchronize()
    return sums, out


@pytest.mark.parametrize("mode", R.MODES)
def test_pointers_that_are_only_4_byte_aligned(dev, mode):
    """Every score and gradient buffer 1, 2, 3 floats past a 16-byte boundary, inside guard bands (tests/misaligned.py): the bits
    of the aligned call (a thread adds the same scores in the same order on either path), nothing written outside the gradients,
    and per-head sums that are the float64 means."""
    import misaligned as MA
    from rave_amd import ops
    sizes = (CHUNK + 8, 260, 5)                  # two workgroups on the 16-byte path, one, and a ragged scalar head
    heads64, _, want_g, mean_abs, head_means = _case(mode, sizes)
    heads = [(r.float().to(dev), f.float().to(dev)) for r, f in heads64]
    g = torch.tensor(GRAD_OUT, device=dev)
    base_g = [(torch.zeros_like(r), torch.zeros_like(f)) for r, f in heads]
    assert all(t.data_ptr() % 256 == 0 for pair in heads + base_g for t in pair)
    sums, out = _raw_call(ops.GAN_MODES[mode], heads, base_g, g, dev)
    for i in range(len(sizes)):
        aten = R.totals(mode, heads[i:i + 1], torch.float32)[0]                  # the float32 ATen composition of this head alone
        for k in range(4):
            bound = max(16 * R.U * (1 + mean_abs[i][k]), 2 * abs(float(aten[k].double().cpu()) - head_means[i][k]))
            assert abs(float(sums[i, k]) - head_means[i][k]) <= bound, (i, k)
        assert rel_l2(torch.cat(base_g[i]), torch.cat(want_g[i])) <= TOL
    for off in (1, 2, 3):
        hs = [(MA.carve(r, off), MA.carve(f, off)) for r, f in heads]
        gs = [(MA.carve(torch.zeros_like(r), off), MA.carve(torch.zeros_like(f), off)) for r, f in heads]
        s2, o2 = _raw_call(ops.GAN_MODES[mode], hs, gs, MA.carve(g, off), dev)
        assert torch.equal(s2, sums) and torch.equal(o2, out), off
        for (a, b), (c, d) in zip(gs, base_g):
            assert torch.equal(a, c) and torch.equal(b, d), off
        assert all(MA.guards_intact(t) for pair in hs + gs for t in pair), off


def _pass(mode, fed_src, dev):
    from rave_amd import ops
    leaves = [t.detach().clone().requires_grad_(True) for t in fed_src]
    out = ops.gan_losses(leaves, mode)
    grads = torch.autograd.grad([out[0], out[1]], leaves, [torch.tensor(v, device=dev) for v in GRAD_OUT])
    return [v.detach() for v in out] + list(grads)


def _unsplit_inputs(mode, dev):
    heads64 = _case(mode, _table_sizes(5))[0]
    return [torch.cat([r.float(), f.float()]).reshape(-1, 1).to(dev) for r, f in heads64]


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_give_the_same_bits(dev, mode):
    src = _unsplit_inputs(mode, dev)
    a, b = _pass(mode, src, dev), _pass(mode, src, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0]) != 0.0


@pytest.mark.parametrize("mode", R.MODES)
def test_recorded_pass_equals_the_eager_one(dev, mode):
    """Forward + backward recorded into a graph after one warm eager call, replayed three times: the bits of the eager call."""
    from rave_amd import ops
    src = _unsplit_inputs(mode, dev)
    leaves = [t.clone().requires_grad_(True) for t in src]
    cot = [torch.tensor(v, device=dev) for v in GRAD_OUT]

    def run():
        out = ops.gan_losses(leaves, mode)
        grads = torch.autograd.grad([out[0]], leaves, [cot[0]])             # one objective only: the other gradient is absent
        return [v.detach() for v in out] + list(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [v.clone() for v in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        recorded = run()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(recorded, eager):
            assert torch.equal(a, b)
    assert all(float(v.abs().max()) > 0 for v in eager[4:])
    del graph


# ---- the training step
N_BAND, N_SIGNAL = 4, 8192       # 2048 band samples: more than half the largest STFT window (16 bands would leave 512)
MODEL_KW = dict(capacity=16, latent_size=16, disc_capacity=16, n_band=N_BAND, update_discriminator_every=2)


def _step(name, batch_idx, switch, dev, monkeypatch):
    """One warmed-up training step from seed-0 weights; returns (logged values, gradients by name, the score maps)."""
    import rave_oracle as O
    from rave_amd import model as M
    monkeypatch.setenv("RH_GAN_LOSS", switch)
    torch.manual_seed(0)
    m = M.build_v2(gan_loss=name, **MODEL_KW).to(dev).train()
    m.configure_optimizers()
    m.warmed_up = True
    seen = []
    inner = m._fused_gan_losses
    m._fused_gan_losses = lambda features: (seen.append([s[-1].detach().clone() for s in features]), inner(features))[1]
    took = []
    from rave_amd import ops
    real = ops.gan_losses
    monkeypatch.setattr(ops, "gan_losses", lambda heads, mode: (took.append(len(heads)), real(heads, mode))[1])
    x = O.synthetic_batch(2, 1, N_SIGNAL, seed=60).to(dev)
    eps = torch.randn(2, 16, N_SIGNAL // (N_BAND * 128), generator=torch.Generator().manual_seed(61)).to(dev)
    logged = m.training_step(x, batch_idx, eps=eps)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "gan_losses", real)
    assert took == ([8] if switch == "1" else [])                 # ONE call over the 8 heads, or none at all
    prefix = "discriminator." if batch_idx % 2 == 0 else "decoder."
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if k.startswith(prefix) and p.grad is not None}
    return {k: torch.as_tensor(v).detach().clone() for k, v in logged.items()}, grads, seen[0]


@pytest.mark.parametrize("name", R.MODES)
def test_training_step_on_the_kernel_and_on_the_composition(dev, name, monkeypatch):
    """A discriminator step (batch 0) and a generator step (batch 1) of the shrunk v2 model, fused against RH_GAN_LOSS=0: the four
    logged scalars of either path against float64 over the step's own score maps (the bound of this file), the gradients of the
    trained half within relative L2 1e-4 of the composition's."""
    for batch_idx in (0, 1):
        lf, gf, heads = _step(name, batch_idx, "1", dev, monkeypatch)
        lc, gc, heads_c = _step(name, batch_idx, "0", dev, monkeypatch)
        assert len(heads) == 8 and all(torch.equal(a, b) for a, b in zip(heads, heads_c))
        pairs = [tuple(t.reshape(-1) for t in torch.split(h.double().cpu(), h.shape[0] // 2, 0)) for h in heads]
        want, _, mean_abs, head_means = R.totals(name, pairs, torch.float64)
        w_adv = 1.0                                               # build_v2's weights["adversarial"]
        for k, key in enumerate(("loss_dis", "adversarial", "pred_real", "pred_fake")):
            assert key in lf and key in lc, key
            scale = w_adv if key == "adversarial" else 1.0
            err_c = abs(float(lc[key]) - scale * float(want[k]))
            err_f = abs(float(lf[key]) - scale * float(want[k]))
            bound = max(R.derived_bound(mean_abs, head_means, k), 2 * err_c)
            print(f"step {name} batch {batch_idx}: {key} fused err {err_f:.3e}, composition err {err_c:.3e}, bound {bound:.3e}")
            assert err_f <= bound, (key, err_f, bound)
        assert set(lf) == set(lc)
        assert len(gf) > 10 and set(gf) == set(gc)
        # (a gradient may be exactly 0 on both paths: with every hinge gate open the last bias gets -n / n + n / n)
        assert sum(float(v.abs().max()) > 0 for v in gc.values()) > 10
        for k in gc:
            assert rel_l2(gf[k], gc[k]) <= TOL, (batch_idx, k, rel_l2(gf[k], gc[k]))


def test_graphed_gan_step_with_ls_replays_the_eager_bits(dev):
    """GraphedTrainingStep over both GAN-phase step kinds with the least-squares objective: the parameters and the logged scalars
    after four replayed steps are those of four eager steps."""
    import rave_oracle as O
    from rave_amd import model as M

    def run(graphed):
        torch.manual_seed(0)
        m = M.build_v2(gan_loss="ls", **MODEL_KW).to(dev).train()
        m.configure_optimizers(capturable=True)
        m.warmed_up = True
        xs = [O.synthetic_batch(2, 1, N_SIGNAL, seed=80 + i).to(dev) for i in range(4)]
        gen = torch.Generator().manual_seed(3)
        es = [torch.randn(2, 16, N_SIGNAL // (N_BAND * 128), generator=gen).to(dev) for _ in range(4)]
        step = M.GraphedTrainingStep(m, xs[0], inject_eps=True) if graphed else None
        logs = []
        for i in range(4):
            if graphed:
                logged = step(xs[i], i, eps=es[i])
            else:
                logged = m.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
            m.on_train_batch_end(None, None, i)
            logs.append({k: torch.as_tensor(v).detach().clone() for k, v in logged.items()})
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.named_parameters()}, logs, (len(step.graphs) if graphed else 2)

    pe, le, _ = run(False)
    pg, lg, kinds = run(True)
    assert kinds == 2
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    for a, b in zip(le, lg):
        assert set(a) == set(b) and {"loss_dis", "adversarial", "pred_real", "pred_fake"} <= set(a)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    torch.manual_seed(0)
    m0 = M.build_v2(gan_loss="ls", **MODEL_KW)
    moved = sum(1 for k, v in m0.named_parameters() if k.startswith("discriminator.") and not torch.equal(v.detach(), pe[k].cpu()))
    assert moved > 5
