"""CPU tests of the GAN objectives (rave/core.py:151-170): the restatement of tests/gan_loss_reference.py against the reference's
own functions (where the reference tree is present) and against the recorded fixture, rave_amd.losses' three functions on CPU
tensors, the refusals of the rh_gan_loss_* entry points (none of which launches anything), the builders' ``gan_loss`` keyword and
the gin overlay."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from functools import partial

import pytest
import torch

import gan_loss_reference as R
from conftest import GOLDEN, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_OUT = (1.0, 0.5)


def _reference_core():
    from ref_import import import_reference, reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    import_reference()
    import rave.core as core
    return core


def _run(fn, r, f, dtype, grad_out=GRAD_OUT):
    r = r.to(dtype).clone().requires_grad_(True)
    f = f.to(dtype).clone().requires_grad_(True)
    dis, adv = fn(r, f)
    (grad_out[0] * dis + grad_out[1] * adv).backward()
    return dis.detach(), adv.detach(), r.grad, f.grad


def _ours():
    from rave_amd import losses
    return {"hinge": losses.hinge_gan, "ls": losses.ls_gan, "nonsaturating": losses.nonsaturating_gan}


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_the_reference_functions(mode):
    """float32: the same expression on the same inputs, saturated scores included -- identical losses and gradients.  float64: on
    scores that stay inside the clamp (the reference's float64 run takes the bounds in float64, the restatement never)."""
    core = _reference_core()
    ref = {"hinge": core.hinge_gan, "ls": core.ls_gan, "nonsaturating": core.nonsaturating_gan}[mode]
    for n in (1, 5, 300):
        r, f = R.scores(n, 7 + n, mode)
        got = _run(partial(R.objective, mode), r, f, torch.float32)
        want = _run(ref, r, f, torch.float32)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (mode, n)
        for k in R.planted(mode, n)["real"]:
            assert float(want[2][k]) == 0.0
        r, f = R.scores(n, 7 + n, mode, plant=False)
        got = _run(partial(R.objective, mode), r, f, torch.float64)
        want = _run(ref, r, f, torch.float64)
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-14 * max(1.0, float(b.abs().max())), (mode, n)


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_the_fixture(mode):
    fx = torch.load(os.path.join(GOLDEN, "gan_loss_tiny.pt"))
    rec = fx[mode]
    assert tuple(fx["grad_out"].tolist()) == GRAD_OUT
    for tag, dtype, tol in (("f32", torch.float32, 0.0), ("f64", torch.float64, 1e-14)):
        dis, adv, dr, df = _run(partial(R.objective, mode), rec["real"], rec["fake"], dtype)
        want = rec[tag]
        assert want["loss_dis"].dtype == dtype and want["d_real"].shape == rec["real"].shape
        for a, b in ((dis, want["loss_dis"]), (adv, want["loss_adv"]), (dr, want["d_real"]), (df, want["d_fake"])):
            assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (mode, tag)
    assert float(rec["f64"]["d_real"].abs().max()) > 0 and float(rec["f64"]["d_fake"].abs().max()) > 0


def test_the_two_new_objectives_exist_with_the_reference_signature():
    import inspect
    from rave_amd import losses
    for name in ("hinge_gan", "ls_gan", "nonsaturating_gan"):
        assert list(inspect.signature(getattr(losses, name)).parameters) == ["score_real", "score_fake"]
    assert [losses.hinge_gan.gan_mode, losses.ls_gan.gan_mode, losses.nonsaturating_gan.gan_mode] == [0, 1, 2]
    assert losses.GAN_LOSSES == {"hinge": losses.hinge_gan, "ls": losses.ls_gan, "nonsaturating": losses.nonsaturating_gan}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("mode", R.MODES)
def test_cpu_functions_equal_the_restatement(mode, dtype):
    """CPU tensors run the torch composition: the restatement's values and gradients (float32: identical; float64: inside the
    clamp, where the bounds do not matter)."""
    r, f = R.scores(300, 21, mode, plant=dtype == torch.float32)
    r, f = r.reshape(2, 1, 150), f.reshape(2, 1, 150)
    got = _run(_ours()[mode], r, f, dtype)
    want = _run(partial(R.objective, mode), r, f, dtype)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == dtype
        assert float((a - b).abs().max()) <= (0.0 if dtype == torch.float32 else 1e-14) * max(1.0, float(b.abs().max()))


def test_hinge_gan_on_cpu_is_the_expression_it_was():
    from rave_amd import losses
    r, f = R.scores(64, 3, "hinge")
    r, f = r.float().reshape(4, 1, 16), f.float().reshape(4, 1, 16)
    dis, adv = losses.hinge_gan(r, f)
    assert torch.equal(dis, (torch.relu(1 - r) + torch.relu(1 + f)).mean()) and torch.equal(adv, -f.mean())
    assert dis.dim() == 0 and adv.dim() == 0


# ---- the C ABI: every refusal happens on the host, before a launch (return code < 0: nothing was enqueued)
def _items(n_items=1, n=8, **override):
    from rave_amd import _lib as L
    arr = (L.GanItem * max(n_items, 1))()
    for a in arr:
        a.real, a.fake, a.d_real, a.d_fake, a.n = 0x1000, 0x2000, 0x3000, 0x4000, n
    for k, v in override.items():
        setattr(arr[0], k, v)
    return arr


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from rave_amd import _lib as L
    lib = L.lib
    ws, sums, out, g = 0x5000, 0x6000, 0x7000, 0x8000
    ok = _items()
    need = lib.rh_gan_loss_workspace_bytes(ok, 1)
    assert need == 4 * 4                                          # one workgroup, four partial sums
    assert lib.rh_gan_loss_workspace_bytes(_items(n=4096), 1) == 16 and lib.rh_gan_loss_workspace_bytes(_items(n=4097), 1) == 32
    assert lib.rh_gan_loss_workspace_bytes(_items(3, n=5000), 3) == 3 * 2 * 16

    def fwd(items=ok, n_items=1, mode=0, ws_=ws, nbytes=need, sums_=sums, out_=out):
        return lib.rh_gan_loss_fwd_f32(items, n_items, mode, ws_, nbytes, sums_, out_, None)

    def bwd(items=ok, n_items=1, mode=0, g_=g):
        return lib.rh_gan_loss_bwd_f32(items, n_items, mode, g_, None)

    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    # null pointers
    assert fwd(items=None) == INVALID and bwd(items=None) == INVALID and lib.rh_gan_loss_workspace_bytes(None, 1) == -1
    for field in ("real", "fake"):
        assert fwd(items=_items(**{field: None})) == INVALID and bwd(items=_items(**{field: None})) == INVALID
        assert b"null" in lib.rh_last_error()
    for field in ("d_real", "d_fake"):
        assert bwd(items=_items(**{field: None})) == INVALID
    assert fwd(ws_=None) == INVALID and fwd(sums_=None) == INVALID and fwd(out_=None) == INVALID and bwd(g_=None) == INVALID
    # n <= 0
    for n in (0, -1):
        assert fwd(items=_items(n=n)) == INVALID and bwd(items=_items(n=n)) == INVALID
        assert lib.rh_gan_loss_workspace_bytes(_items(n=n), 1) == -1
    # n_items outside 1 ... 80
    big = _items(81)
    for n_items in (0, -1, 81):
        assert fwd(items=big, n_items=n_items, nbytes=1 << 20) == UNSUPPORTED and bwd(items=big, n_items=n_items) == UNSUPPORTED
        assert lib.rh_gan_loss_workspace_bytes(big, n_items) == -1
    assert lib.rh_gan_loss_workspace_bytes(big, 80) == 80 * 16
    # an unknown mode
    for mode in (-1, 3, 99):
        assert fwd(mode=mode) == UNSUPPORTED and bwd(mode=mode) == UNSUPPORTED
        assert b"mode" in lib.rh_last_error()
    # a workspace that is too small
    assert fwd(nbytes=need - 1) == WORKSPACE and fwd(nbytes=0) == WORKSPACE
    assert fwd(items=_items(n=4097), nbytes=16) == WORKSPACE
    with pytest.raises(RuntimeError, match="workspace"):
        L.check(fwd(nbytes=0), "gan_loss_fwd")


def test_supported_gives_the_documented_table():
    from rave_amd import _lib as L
    for mode in range(-2, 6):
        for n_items in (-1, 0, 1, 2, 79, 80, 81, 1000):
            assert L.lib.rh_gan_loss_supported(mode, n_items) == int(mode in (0, 1, 2) and 1 <= n_items <= 80), (mode, n_items)
    assert (L.GAN_HINGE, L.GAN_LS, L.GAN_NONSAT) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "rave_hip.h")).read()
    for name, val in (("RH_GAN_HINGE", 0), ("RH_GAN_LS", 1), ("RH_GAN_NONSAT", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr)
    assert C.sizeof(L.GanItem) == 40


def test_ops_raise_on_cpu_and_on_float64_tensors():
    from rave_amd import ops
    r, f = torch.zeros(4, 1, 8), torch.zeros(4, 1, 8)
    for mode in R.MODES:
        with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
            ops.gan_losses([torch.cat([r, f])], mode)
        with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
            ops.gan_losses([(r, f)], mode)
        with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
            ops.gan_losses([(r.double(), f.double())], mode)
    with pytest.raises(ValueError, match="mode"):
        ops.gan_losses([(r, f)], "wasserstein")
    with pytest.raises(RuntimeError, match="no heads"):
        ops.gan_losses([], "hinge")


def test_switch_reads_the_environment(monkeypatch):
    from rave_amd import ops
    monkeypatch.delenv("RH_GAN_LOSS", raising=False)
    assert ops.gan_loss_on()
    monkeypatch.setenv("RH_GAN_LOSS", "0")
    assert not ops.gan_loss_on()
    monkeypatch.setenv("RH_GAN_LOSS", "1")
    assert ops.gan_loss_on()


def test_builders_take_the_objective_by_name():
    from rave_amd import losses
    from rave_amd import model as M
    kw = dict(capacity=16, latent_size=16, disc_capacity=16)
    with pytest.raises(ValueError, match="gan_loss"):
        M.build_v2(gan_loss="wasserstein", **kw)
    torch.manual_seed(0)
    base = M.build_v2(**kw)
    assert base.gan_loss is losses.hinge_gan
    sd0 = base.state_dict()
    for name, fn in losses.GAN_LOSSES.items():
        torch.manual_seed(0)
        m = M.build_v2(gan_loss=name, **kw)
        assert m.gan_loss is fn
        sd = m.state_dict()
        assert list(sd) == list(sd0) and all(torch.equal(sd[k], sd0[k]) for k in sd0)
    assert M.build_v3(gan_loss="ls", spectral_capacity=8, **kw).gan_loss is losses.ls_gan
    assert M.build_discrete(gan_loss="nonsaturating", spectral_capacity=8, **kw).gan_loss is losses.nonsaturating_gan


def test_step_recognises_the_objective(monkeypatch):
    """By identity, through an argument-free ``partial``, and through the ``gan_mode`` attribute a wrapper carries over
    (functools.wraps, what gin's wrappers do); anything else, CPU score maps and RH_GAN_LOSS=0 take the per-head loop."""
    import functools
    from rave_amd import losses, ops
    from rave_amd import model as M
    monkeypatch.setenv("RH_GAN_LOSS", "1")
    m = M.build_v2(capacity=16, latent_size=16, disc_capacity=16)
    feats = [[torch.zeros(4, 1, 8)], [torch.zeros(4, 1, 8)]]
    assert m._fused_gan_losses(feats) is None                     # CPU maps
    seen = []
    monkeypatch.setattr(ops, "gan_losses",
                        lambda heads, mode: (seen.append((len(heads), mode)), tuple(torch.zeros(()) for _ in range(4)))[1])

    class FakeCuda(torch.Tensor):                                 # a host tensor that answers is_cuda: only the choice is tested
        is_cuda = True
    cuda_feats = [[torch.zeros(4, 1, 8).as_subclass(FakeCuda)] for _ in range(3)]

    @functools.wraps(losses.ls_gan)
    def wrapped(a, b):
        return losses.ls_gan(a, b)

    for fn, mode in ((losses.hinge_gan, 0), (partial(losses.nonsaturating_gan), 2), (wrapped, 1)):
        m.gan_loss = fn
        assert m._fused_gan_losses(cuda_feats) is not None and seen[-1] == (3, mode)
    n = len(seen)
    for fn in (lambda a, b: losses.hinge_gan(a, b), partial(losses.hinge_gan, score_fake=None)):
        m.gan_loss = fn
        assert m._fused_gan_losses(cuda_feats) is None
    m.gan_loss = losses.hinge_gan
    monkeypatch.setenv("RH_GAN_LOSS", "0")
    assert m._fused_gan_losses(cuda_feats) is None
    monkeypatch.setenv("RH_GAN_LOSS", "1")
    odd = [[torch.zeros(3, 1, 8).as_subclass(FakeCuda)]]
    assert m._fused_gan_losses(odd) is None                       # an odd batch dimension cannot be halved
    assert len(seen) == n


# ---- the gin overlay
def test_overlay_parses_and_binds_existing_names():
    import importlib
    import inspect
    text = open(os.path.join(ROOT, "rave_amd", "configs", "mi355x_gan_loss.gin")).read()
    code = [ln for ln in text.splitlines() if ln.strip() and not ln.lstrip().startswith("#")]
    assert code == ["from __gin__ import dynamic_registration", "import rave", "import rave_amd.losses", "rave.RAVE:",
                    "    gan_loss = @rave_amd.losses.hinge_gan"]
    header = [ln for ln in text.splitlines() if ln.startswith("#")]
    shown = re.findall(r"gan_loss = @([\w.]+)", "\n".join(header))
    assert shown == ["rave_amd.losses.hinge_gan", "rave_amd.losses.ls_gan", "rave_amd.losses.nonsaturating_gan"]
    for ref in shown:
        mod, name = ref.rsplit(".", 1)
        fn = getattr(importlib.import_module(mod), name)
        assert callable(fn) and list(inspect.signature(fn).parameters) == ["score_real", "score_fake"]


_GIN_SCRIPT = r"""
import json, os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle"))
sys.dont_write_bytecode = True
from ref_import import import_reference
rave = import_reference()
import gin, torch
from rave_amd import losses
res = {}
for name in ("hinge_gan", "ls_gan", "nonsaturating_gan"):
    gin.clear_config()
    cfg = os.path.join(root, "rave_amd", "configs")
    text = open(os.path.join(cfg, "mi355x_gan_loss.gin")).read().replace("= @rave_amd.losses.hinge_gan\n", "= @rave_amd.losses.%s\n" % name)
    assert text.count("@rave_amd.losses.%s\n" % name) >= 1
    gin.parse_config_files_and_bindings(["configs/v2.gin", os.path.join(cfg, "mi355x.gin")], ["CAPACITY = 8", "LATENT_SIZE = 16"])
    gin.parse_config(text)
    model = rave.RAVE()                       # upstream's own class, every argument from the parsed .gin files
    fn = model.gan_loss
    target = getattr(fn, "__gin_target__", getattr(fn, "__wrapped__", fn))
    r, f = torch.randn(2, 1, 9), torch.randn(2, 1, 9)
    same = all(torch.equal(a, b) for a, b in zip(fn(r, f), getattr(losses, name)(r, f)))
    res[name] = dict(cls=type(model).__module__, is_dropin=target is getattr(losses, name), same=same)
print("RESULT" + json.dumps(res))
"""


def test_overlay_hands_the_drop_in_function_to_upstreams_model():
    """v2 + mi355x.gin + the overlay (and the overlay with each of the other two choices of its header bound instead): the
    unmodified ``rave.RAVE`` holds the rave_amd.losses function.  (Construction only; needs upstream's package.)"""
    _reference_core()
    r = subprocess.run([sys.executable, "-c", _GIN_SCRIPT, ROOT], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert set(res) == {"hinge_gan", "ls_gan", "nonsaturating_gan"}
    for name, v in res.items():
        assert v == dict(cls="rave.model", is_dropin=True, same=True), (name, v)


def test_header_exports_are_dynamic_symbols_of_the_library():
    """Every rh_* function include/rave_hip.h declares -- the four new ones among them -- is a dynamic symbol of the library."""
    from rave_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rave_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rh_[a-z0-9_]+)\s*\(", src))
    new = {"rh_gan_loss_supported", "rh_gan_loss_workspace_bytes", "rh_gan_loss_fwd_f32", "rh_gan_loss_bwd_f32"}
    assert new <= declared
    for n in sorted(declared):
        assert hasattr(L.lib, n), f"librave_hip.so does not export {n}"
    assert re.search(r"rave/core\.py:151-170", open(os.path.join(ROOT, "include", "rave_hip.h")).read())
    assert re.search(r"rave/model\.py:354-376", open(os.path.join(ROOT, "include", "rave_hip.h")).read())
