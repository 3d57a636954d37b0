"""The weight average of `rave train --ema` on the GPU (rave_amd/csrc/ema.hip, rave_amd/ema.py) against the reference's
callback (scripts/train.py:81-120) restated with torch operators: the two kernels through the C ABI, the callback's
semantics, eager and graphed training, and that validation really runs the averaged weights.  Every comparison is
``torch.equal``: the kernel performs the reference's three roundings (tests/test_ema_host.py shows that these inputs tell
them from any contraction)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rave_oracle as O  # noqa: E402  (input batches only)

from ema_cases import FACTORS, GUARD, P_MISALIGNED, SIZES, W_MISALIGNED, ema_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD_VALUE = -77.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def reference_update(weights, named, factor):
    """scripts/train.py:88-96, restated."""
    for n, p in named:
        if n not in weights:
            weights[n] = p.data.clone()
            continue
        weights[n] = weights[n] * factor + p.data * (1 - factor)


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------

class PairTable:
    """The 70 tensor pairs of ema_cases on the GPU, every one inside its own guarded buffer; two of them start one float
    past a 16-byte boundary (one on each side)."""

    def __init__(self, dev):
        from rave_amd import _lib as L
        self.host = ema_inputs()
        self.bufs, self.views = [], []
        self.items = (L.PairItem * len(SIZES))()
        for i, (w, p) in enumerate(self.host):
            n = w.numel()
            offs = (GUARD + (i == W_MISALIGNED), GUARD + (i == P_MISALIGNED))
            bufs = tuple(torch.full((n + 2 * GUARD + 1,), GUARD_VALUE, device=dev) for _ in offs)
            views = tuple(b[o:o + n] for b, o in zip(bufs, offs))
            for v, o in zip(views, offs):
                assert v.data_ptr() % 16 == 4 * (o - GUARD)
            self.bufs.append(bufs)
            self.views.append(views)
            self.items[i].a, self.items[i].b, self.items[i].n = views[0].data_ptr(), views[1].data_ptr(), n
        self.fill()

    def fill(self):
        for (w, p), (wv, pv) in zip(self.host, self.views):
            wv.copy_(w)
            pv.copy_(p)

    def guards_intact(self):
        for (wb, pb), (wv, pv) in zip(self.bufs, self.views):
            for b, v in ((wb, wv), (pb, pv)):
                o = v.storage_offset()
                if not (bool((b[:o] == GUARD_VALUE).all()) and bool((b[o + v.numel():] == GUARD_VALUE).all())):
                    return False
        return True


@pytest.fixture(scope="module")
def table(dev):
    return PairTable(dev)


@pytest.mark.parametrize("factor", FACTORS)
def test_ema_update_is_bit_identical_to_the_torch_expression(table, factor):
    from rave_amd import _lib as L
    table.fill()
    want = [w * factor + p * (1 - factor) for w, p in table.views]
    L.check(L.lib.rh_ema_update_f32(table.items, len(SIZES), factor, L.stream()), "ema_update")
    torch.cuda.synchronize()
    for i, ((w, p), (_, p0)) in enumerate(zip(table.views, table.host)):
        assert torch.equal(w, want[i]), (i, SIZES[i])
        assert torch.equal(p.cpu(), p0), (i, SIZES[i])                  # the parameter side is only read
    assert table.guards_intact()


def test_swap_exchanges_both_sides_and_a_second_swap_restores_them(table):
    from rave_amd import _lib as L
    table.fill()
    L.check(L.lib.rh_swap_f32(table.items, len(SIZES), L.stream()), "swap")
    torch.cuda.synchronize()
    for i, ((w, p), (w0, p0)) in enumerate(zip(table.views, table.host)):
        assert torch.equal(w.cpu(), p0) and torch.equal(p.cpu(), w0), (i, SIZES[i])
    assert table.guards_intact()
    L.check(L.lib.rh_swap_f32(table.items, len(SIZES), L.stream()), "swap")
    torch.cuda.synchronize()
    for i, ((w, p), (w0, p0)) in enumerate(zip(table.views, table.host)):
        assert torch.equal(w.cpu(), w0) and torch.equal(p.cpu(), p0), (i, SIZES[i])
    assert table.guards_intact()


# ---- the callback ------------------------------------------------------------------------------------------------------

def test_callback_semantics_on_a_plain_module(dev):
    from rave_amd.ema import EMA
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).to(dev)
    names = [n for n, _ in net.named_parameters()]
    gen = torch.Generator().manual_seed(4)

    def perturb():
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.01 * torch.randn(p.shape, generator=gen).to(dev))

    ema, ref = EMA(.999), {}
    ema.on_train_batch_end(None, net, None, None, 0)
    reference_update(ref, net.named_parameters(), .999)
    assert list(ema.weights) == names
    for n, p in net.named_parameters():                                  # the first call clones and does not average
        assert torch.equal(ema.weights[n], p.data) and ema.weights[n].data_ptr() != p.data_ptr()
    for i in range(1, 6):
        perturb()
        ema.on_train_batch_end(None, net, None, None, i)
        reference_update(ref, net.named_parameters(), .999)
    for n in names:
        assert torch.equal(ema.weights[n], ref[n]), n
        assert not torch.equal(ref[n], dict(net.named_parameters())[n].data), n

    # a checkpoint's callback state (CPU tensors) into a fresh object, one more update: the uninterrupted run
    sd = ema.state_dict()
    assert sd is not ema.weights and list(sd) == names and all(sd[n] is ema.weights[n] for n in names)
    resumed = EMA(.999)
    resumed.load_state_dict({n: v.cpu() for n, v in sd.items()})
    perturb()
    ema.on_train_batch_end(None, net, None, None, 6)
    resumed.on_train_batch_end(None, net, None, None, 6)
    reference_update(ref, net.named_parameters(), .999)
    for n in names:
        assert resumed.weights[n].device == dev and torch.equal(resumed.weights[n], ema.weights[n]), n
        assert torch.equal(ema.weights[n], ref[n]), n
    # load_state_dict copies INTO the averages it already holds
    ptrs = {n: resumed.weights[n].data_ptr() for n in names}
    resumed.load_state_dict({n: torch.zeros_like(v).cpu() for n, v in sd.items()})
    assert all(resumed.weights[n].data_ptr() == ptrs[n] and not bool(resumed.weights[n].any()) for n in names)

    # swap_weights exchanges contents in place: nothing is rebound
    before = {n: (p.data.clone(), ema.weights[n].clone(), p.data_ptr(), ema.weights[n].data_ptr(), p._version)
              for n, p in net.named_parameters()}
    ema.swap_weights(net)
    for n, p in net.named_parameters():
        pv, wv, pp, wp, ver = before[n]
        assert torch.equal(p.data, wv) and torch.equal(ema.weights[n], pv), n
        assert p.data_ptr() == pp and ema.weights[n].data_ptr() == wp, n
        assert p._version > ver, n                                       # version-keyed caches see the swap
    ema.swap_weights(net)
    for n, p in net.named_parameters():
        assert torch.equal(p.data, before[n][0]) and torch.equal(ema.weights[n], before[n][1]), n


def test_validation_hooks_without_averages_say_so(dev, capsys):
    from rave_amd.ema import EMA
    net = torch.nn.Linear(3, 2).to(dev)
    w = net.weight.data.clone()
    ema = EMA()
    ema.on_validation_epoch_start(None, net)
    ema.on_validation_epoch_end(None, net)
    assert capsys.readouterr().out == "no ema weights available\n" * 2 and torch.equal(net.weight.data, w)


def test_unsupported_parameters_are_refused(dev):
    from rave_amd.ema import EMA
    with pytest.raises(RuntimeError, match="GPU"):
        EMA().on_train_batch_end(None, torch.nn.Linear(3, 2), None, None, 0)
    lin = torch.nn.Linear(4, 3).to(dev)
    lin.weight = torch.nn.Parameter(torch.randn(4, 3, device=dev).t())
    assert not lin.weight.is_contiguous()
    with pytest.raises(RuntimeError, match="GPU"):
        EMA().on_train_batch_end(None, lin, None, None, 0)
    ema = EMA()
    ema.weights = {n: p.data.clone().contiguous() for n, p in lin.named_parameters()}
    with pytest.raises(RuntimeError, match="GPU"):
        ema.swap_weights(lin)


# ---- training ----------------------------------------------------------------------------------------------------------

STEPS = 4
FACTOR = .999


def _train(dev, graphed, with_ema):
    """4 alternating GAN-phase steps (discriminator / generator) of the shrunk v2 model, as tests/test_gpu_dispatch.py's
    graphed-vs-eager test runs them; parameters snapshotted after every step."""
    from rave_amd import model as M
    from rave_amd.ema import EMA
    torch.manual_seed(0)
    m = M.build_v2(capacity=16, latent_size=16, disc_capacity=16, update_discriminator_every=2).to(dev).train()
    m.configure_optimizers(capturable=True)
    m.warmed_up = True
    xs = [O.synthetic_batch(2, 1, 32768, seed=70 + i).to(dev) for i in range(STEPS)]
    gen = torch.Generator().manual_seed(2)
    es = [torch.randn(2, 16, 16, generator=gen).to(dev) for _ in range(STEPS)]
    step = M.GraphedTrainingStep(m, xs[0], inject_eps=True) if graphed else None
    ema = EMA(FACTOR) if with_ema else None
    snaps = []
    for i in range(STEPS):
        if graphed:
            step(xs[i], i, eps=es[i])
        else:
            m.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
        m.on_train_batch_end(None, None, i)
        if ema is not None:
            ema.on_train_batch_end(None, m, None, None, i)
        snaps.append({k: v.detach().clone() for k, v in m.named_parameters()})
    torch.cuda.synchronize()
    weights = {k: v.clone() for k, v in ema.weights.items()} if with_ema else None
    return dict(model=m, ema=ema, snaps=snaps, weights=weights, x=xs[0], eps=es[0])


@pytest.fixture(scope="module")
def eager(dev):
    return _train(dev, graphed=False, with_ema=True)


def test_eager_training_averages_every_parameter(eager):
    snaps, weights = eager["snaps"], eager["weights"]
    names = list(snaps[0])
    assert list(weights) == names
    ref = {}
    for snap in snaps:
        reference_update(ref, snap.items(), FACTOR)
    for n in names:
        assert torch.equal(weights[n], ref[n]), n
    # generator, discriminator and parameters no optimizer owns (the PQMF bank) are all averaged
    for prefix in ("encoder.", "decoder.", "discriminator.", "pqmf."):
        assert any(n.startswith(prefix) for n in names), prefix
    moved = [n for n in names if not torch.equal(snaps[0][n], snaps[-1][n])]
    assert any(n.startswith("decoder.") for n in moved) and any(n.startswith("discriminator.") for n in moved)
    for n in moved:                                                      # ... and the average lags behind the parameters
        assert not torch.equal(weights[n], snaps[-1][n]), n


def test_graphed_training_is_bit_identical_and_undisturbed(dev, eager):
    graphed = _train(dev, graphed=True, with_ema=True)
    for n, v in eager["snaps"][-1].items():
        assert torch.equal(graphed["snaps"][-1][n], v), n
        assert torch.equal(graphed["weights"][n], eager["weights"][n]), n
    del graphed
    plain = _train(dev, graphed=True, with_ema=False)
    for n, v in eager["snaps"][-1].items():
        assert torch.equal(plain["snaps"][-1][n], v), n


def test_validation_sees_the_averaged_weights(dev, eager):
    from rave_amd import model as M
    m, ema, x, eps = eager["model"], eager["ema"], eager["x"], eager["eps"]
    params, weights = eager["snaps"][-1], eager["weights"]
    m.eval()
    try:
        with torch.no_grad():
            y_pre = m.validation_step(x, 0, eps=eps)[0].clone()          # (leaves the packed weights cached)
            ema.on_validation_epoch_start(None, m)
            y_avg = m.validation_step(x, 0, eps=eps)[0].clone()
            # a second, freshly built model that was GIVEN the averages the ordinary way
            torch.manual_seed(0)
            m2 = M.build_v2(capacity=16, latent_size=16, disc_capacity=16, update_discriminator_every=2).to(dev).eval()
            m2.warmed_up = True
            res = m2.load_state_dict({**dict(m.named_buffers()), **weights}, strict=False)
            assert not [k for k in res.missing_keys if k in weights]
            for n, p in m2.named_parameters():
                assert torch.equal(p.data, weights[n]), n
            y_ref = m2.validation_step(x, 0, eps=eps)[0]
            assert torch.equal(y_avg, y_ref)
            assert not torch.equal(y_avg, y_pre)
            for n, p in m.named_parameters():
                assert torch.equal(p.data, weights[n]) and torch.equal(ema.weights[n], params[n]), n
            ema.on_validation_epoch_end(None, m)
            for n, p in m.named_parameters():
                assert torch.equal(p.data, params[n]) and torch.equal(ema.weights[n], weights[n]), n
            y_post = m.validation_step(x, 0, eps=eps)[0]
            assert torch.equal(y_post, y_pre)
    finally:
        m.train()
