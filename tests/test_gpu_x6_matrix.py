"""Every row of the conv_x6_kernel instance matrix (tests/x6_matrix.py) as ONE direct C-ABI call, checked four ways:

a. against a plain f64 evaluation on the CPU (F.conv1d / F.conv_transpose1d on the activated input, plus bias, add and output
   activation; the data gradient is the autograd of that expression), relative L2 below TOL_OP -- the tolerance of
   test_gpu_parity.py: test_conv1d_fwd_and_grads_vs_cpu -- on the whole tensor AND on every edge slice (last batch item, last
   32-row block, last column tile of every item, the padded first / last columns, each output phase of the strided forms), so that
   an error confined to one tile edge is not averaged away;
b. against the f32-input MFMA family on the same operands (RH_CONV_X6=0, read per call), below the 2e-6 of the shadow check of
   test_gpu_dispatch.py, on the same slices;
c. guard words around the output untouched; after a call that was offered a workspace, the words behind
   rh_conv1d_*_workspace_bytes untouched;
d. the instance key is real on the device: a row split in K ("combine", "finalize") has written partial sums into the zeroed
   workspace (the launcher runs unsplit, silently, with an unusable one), and a row of 4096 outputs or more differs in bits from
   its f32-input MFMA result (the planner takes those kernels, silently, when the input's range slot is not armed).
Both tolerances are the project's existing ones; nothing here is a new measurement.  tests/test_x6_matrix_host.py pins which
instance each row launches; a mode the planner accepts and x6_launch lacks fails the call itself (RH_ERR_UNSUPPORTED).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import x6_matrix as X
from conftest import rel_l2
from misaligned import _Env, carve, guards_intact

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5       # tests/test_gpu_parity.py
TOL_SHADOW = 2e-6   # tests/test_gpu_dispatch.py: x6 against the f32-input MFMA kernels, per launch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    X.assert_default_planner_env()
    return _ops


def _operands(row):
    """Host operands of a row: randn scaled so that no output is near zero in norm, and one large element in the last input
    channel at the last position of the last batch item (only the last K slice and the last column tile see it)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    gen = torch.Generator().manual_seed(X.seed(row.name))
    lo = X.out_len(row.geo)
    t = dict(x=torch.randn(B, Ci, Lx, generator=gen),
             w=(torch.randn(Ci, Co, k, generator=gen) if tr else torch.randn(Co, Ci, k, generator=gen)) / math.sqrt(Ci * k))
    if row.which == 0:
        t["x"][-1, -1, -1] = 40.0
        if "b" in row.ops:
            t["b"] = torch.randn(Co, generator=gen)
        if "a" in row.ops:
            t["add"] = torch.randn(B, Co, lo, generator=gen)
    else:
        t["dy"] = torch.randn(B, Co, lo, generator=gen)
        t["dy"][-1, -1, -1] = 40.0
        if "a" in row.ops:
            t["add"] = torch.randn(B, Ci, Lx, generator=gen)
    return t


def _reference(row, t):
    """f64 on the CPU."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    lo = X.out_len(row.geo)
    x = t["x"].double().requires_grad_(row.which == 1)
    w = t["w"].double()
    xa = F.leaky_relu(x, X.SLOPE) if "L" in row.ops else x
    if tr:
        y = F.conv_transpose1d(xa, w, stride=s, padding=pad[0])
        assert y.shape[-1] == lo
    else:
        y = F.conv1d(F.pad(xa, pad), w, stride=s, dilation=dil)
        assert y.shape[-1] == lo
    if row.which == 1:
        (dx,) = torch.autograd.grad(y, x, t["dy"].double())
        return dx + t["add"].double() if "add" in t else dx
    if "b" in t:
        y = y + t["b"].double().view(1, -1, 1)
    if "add" in t:
        y = y + t["add"].double()
    return F.leaky_relu(y, X.OUT_SLOPE) if "o" in row.ops else y


def _slices(row, info, shape):
    """(name, index) of the edge slices of the output tensor (B, M, n)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    Bn, M, n = shape
    sl = [("whole", (slice(None),) * 3), ("last batch item", (slice(Bn - 1, Bn),)), ("last 32-row block", (slice(None), slice((M - 1) // 32 * 32, M)))]
    strided = (row.which == 0 and tr) or (row.which == 1 and not tr)         # s output phases (virtual rows or grid phases)
    per = s if strided and s > 1 else 1
    if info[0] == 1:
        g = X.tile_geometry(row, info)
        first = (g["tiles_per_b"] - 1) * g["bnl"] * per                      # first output column of the last column tile
        sl.append(("last column tile", (slice(None), slice(None), slice(min(first, n - 1), n))))
    if pad[0] > 0:
        sl.append(("first pad_left columns", (slice(None), slice(None), slice(0, min(n, pad[0])))))
    if pad[1] > 0:
        sl.append(("last pad_right columns", (slice(None), slice(None), slice(max(0, n - pad[1]), n))))
    if per > 1:
        sl += [(f"output phase {j}", (slice(None), slice(None), slice(j, n, per))) for j in range(min(per, n))]
    return sl


def _compare(what, got, ref, slices, tol):
    for name, idx in slices:
        a, b = got[idx], ref[idx]
        if b.numel() == 0:
            continue
        err = rel_l2(a, b)
        print(f"  {what} {name}: rel L2 {err:.3e} (bound {tol:g})")
        assert err < tol, (what, name, err, tol)


@pytest.mark.parametrize("row", X.ROWS, ids=[r.name for r in X.ROWS])
def test_row(ops, dev, row):
    L = ops.L
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    lo = X.out_len(row.geo)
    key = X.derive_key(L, row)
    assert key == row.key, (X.fmt_key(key), X.fmt_key(row.key))
    info = X.plan_info(L, row)
    d = X.desc(L, row)
    t = _operands(row)
    ref = _reference(row, t).detach()
    assert float(ref.norm()) / math.sqrt(ref.numel()) > 0.1                   # no output near zero in norm
    g = {n: v.to(dev) for n, v in t.items()}
    st = L.stream()
    wp_f = torch.empty(L.lib.rh_conv1d_packed_floats(C.byref(d), 0), device=dev)
    wp_b = torch.empty(L.lib.rh_conv1d_packed_floats(C.byref(d), 1), device=dev)
    L.check(L.lib.rh_conv1d_pack_f32(C.byref(d), L.ptr(g["w"]), L.ptr(wp_f), L.ptr(wp_b), st), "pack")
    src = g["x"] if row.which == 0 else g["dy"]
    out_shape = (B, Co, lo) if row.which == 0 else (B, Ci, Lx)
    nbytes = X.workspace_bytes(L, row) if row.ws else 0
    assert nbytes >= 0

    def call(x6):
        out = carve(torch.zeros(out_shape, device=dev), 0)
        ws = carve(torch.zeros(nbytes // 4, device=dev), 0) if nbytes > 0 else None
        rin = torch.zeros(ops._RANGE_WORDS, device=dev, dtype=torch.int32)
        rout = torch.zeros(ops._RANGE_WORDS, device=dev, dtype=torch.int32)
        L.check(L.lib.rh_amax_f32(L.ptr(src), src.numel(), L.ptr(rin), st), "amax")
        with _Env(RH_CONV_X6=None if x6 else 0, RH_X6_COMBINE=row.combine):
            L.lib.rh_x6_set_ranges(None, L.ptr(rin) if x6 else None, L.ptr(rout), None)
            if row.which == 0:
                rc = L.lib.rh_conv1d_fwd_f32(C.byref(d), L.ptr(g["x"]), L.ptr(wp_f), L.ptr(g.get("b")), None, L.ptr(g.get("add")),
                                             L.ptr(out), L.ptr(ws), nbytes, st)
            else:
                rc = L.lib.rh_conv1d_bwd_data_f32(C.byref(d), L.ptr(g["dy"]), L.ptr(wp_b), L.ptr(g["x"]), None, L.ptr(g.get("add")),
                                                  L.ptr(out), L.ptr(ws), nbytes, st)
        L.check(rc, row.name)
        torch.cuda.synchronize()
        assert guards_intact(out), "guard words around the output were written"
        if ws is not None:
            assert guards_intact(ws), "the workspace was written beyond rh_conv1d_*_workspace_bytes"
        if x6 and row.key is not None and row.key.kmode in ("combine", "finalize"):
            assert ws is not None and bool((ws != 0).any()), "planned split in K, but no partial sum reached the workspace"
        assert torch.isfinite(out).all()
        if x6:
            assert float(rout.view(torch.float32).max()) >= float(out.abs().max())   # (the published range covers the output)
        return out.cpu()

    got = call(True)
    print(f"{row.name}: {X.fmt_key(row.key)}")
    slices = _slices(row, info, out_shape)
    _compare("vs f64", got, ref, slices, TOL_OP)
    if row.key is not None:
        f32 = call(False)
        _compare("vs f32-input MFMA", got, f32, slices, TOL_SHADOW)
        if got.numel() >= 4096:      # two f16 pieces per input against f32 inputs: the same bits throughout = the same kernels ran
            assert not torch.equal(got, f32), "the conv_x6_kernel result equals the f32-input MFMA result bit for bit"
