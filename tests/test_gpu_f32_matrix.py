"""Every row of the f32-input MFMA instance matrix (tests/f32_matrix.py) as ONE direct C-ABI call with no range slot armed, every
pointer carved at the row's alignment (tests/misaligned.py), checked four ways:

a. against a plain f64 evaluation on the CPU (F.conv1d / F.conv_transpose1d on the activated input -- Snake is
   x + sin^2(alpha x) / (alpha + 1e-9) --, the (k,1) fold form as a 2-D convolution, then bias, add and output activation; the data
   gradient is the autograd of that expression), relative L2 below TOL_OP -- the tolerance test_gpu_parity.py already holds these
   kernels to -- on the whole tensor AND on every edge slice (last batch item, last 32-row block, last column tile of every item,
   the padded first / last columns, each output phase, each ``inner`` lane, the columns the large element of the last K chunk
   feeds), so that an error confined to one tile edge is not averaged away;
b. guard words around the output untouched; the words behind rh_conv1d_*_workspace_bytes untouched;
c. the key is real on the device: a "finalize" / "finalize4" row has written partial sums into the zeroed workspace, a "nows" row
   is offered none;
d. "same accumulation order per output" (conv_igemm_dma.hip): a VEC row and its 4-byte-aligned twin (the element-wise variant)
   agree bit for bit whenever rh_conv1d_f32_instance_info reports the same ck, K slices and tile shape for both.
tests/test_f32_matrix_host.py pins which instance each row launches.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import f32_matrix as X
from conftest import rel_l2
from misaligned import carve, guards_intact

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5       # tests/test_gpu_parity.py


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
    channel at the last position of the last batch item (only the last K chunk and the last column tile see it)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    gen = torch.Generator().manual_seed(X.seed(row.name))
    g = X.gemm(row)
    x_row, y_row = (g["in_row"], g["out_row"]) if row.which == 0 else (g["out_row"], g["in_row"])
    t = dict(x=torch.randn(B, Ci, x_row, generator=gen),
             w=(torch.randn(Ci, Co, k, generator=gen) if tr else torch.randn(Co, Ci, k, generator=gen)) / math.sqrt(Ci * k))
    if "S" in row.ops:
        t["alpha"] = 0.5 + torch.rand(Ci, generator=gen)
    if row.which == 0:
        t["x"][-1, -1, -1] = 40.0
        if "b" in row.ops:
            t["b"] = torch.randn(Co, generator=gen)
        if "a" in row.ops:
            t["add"] = torch.randn(B, Co, y_row, generator=gen)
    else:
        t["dy"] = torch.randn(B, Co, y_row, generator=gen)
        t["dy"][-1, -1, -1] = 40.0
        if "a" in row.ops:
            t["add"] = torch.randn(B, Ci, x_row, generator=gen)
    return t


def _reference(row, t, big=True):
    """f64 on the CPU (``big`` = False: without the one large element)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    lo = X.out_len(row.geo)
    src = {n: v.double().clone() for n, v in t.items()}
    if not big:
        src["x" if row.which == 0 else "dy"][-1, -1, -1] = 0.0
    x = src["x"].requires_grad_(row.which == 1)
    xf = F.pad(x, (0, Lx * inner - x.shape[-1]))                              # the fold's zero padding behind in_valid
    if "S" in row.ops:
        a = src["alpha"].view(1, -1, 1)
        xa = xf + torch.sin(a * xf) ** 2 / (a + 1e-9)
    else:
        xa = F.leaky_relu(xf, X.SLOPE) if "L" in row.ops else xf
    if tr:
        y = F.conv_transpose1d(xa, src["w"], stride=s, padding=pad[0])
    elif inner == 1:
        y = F.conv1d(F.pad(xa, pad), src["w"], stride=s, dilation=dil)
    else:
        x2 = F.pad(xa.view(B, Ci, Lx, inner), (0, 0) + tuple(pad))
        y = F.conv2d(x2, src["w"].unsqueeze(-1), stride=(s, 1), dilation=(dil, 1)).reshape(B, Co, -1)
    assert y.shape[-1] == lo * inner
    if row.which == 1:
        (dx,) = torch.autograd.grad(y, x, src["dy"])
        return (dx + src["add"] if "add" in src else dx).detach()
    if "b" in src:
        y = y + src["b"].view(1, -1, 1)
    if "add" in src:
        y = y + src["add"]
    return (F.leaky_relu(y, X.OUT_SLOPE) if "o" in row.ops else y).detach()


def _slices(row, info, ref, ref_small):
    """(name, index) of the edge slices of the output tensor (B, M, n)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    Bn, M, n = ref.shape
    g = X.gemm(row)
    per = g["ostr"]
    sl = [("whole", (slice(None),) * 3), ("last batch item", (slice(Bn - 1, Bn),)), ("last 32-row block", (slice(None), slice((M - 1) // 32 * 32, M)))]
    first = (info.tiles_per_b - 1) * info.bnl // inner * per * inner                 # first output element of the last column tile
    sl.append(("last column tile", (slice(None), slice(None), slice(min(first, n - 1), n))))
    if pad[0] > 0:
        sl.append(("first pad_left columns", (slice(None), slice(None), slice(0, min(n, pad[0] * inner)))))
    if pad[1] > 0:
        sl.append(("last pad_right columns", (slice(None), slice(None), slice(max(0, n - pad[1] * inner), n))))
    if per > 1:
        rows = torch.arange(n) // inner
        sl += [(f"output phase {j}", (slice(None), slice(None), rows % per == j)) for j in range(per)]
    if inner > 1:
        sl += [(f"inner lane {j}", (slice(None), slice(None), slice(j, n, inner))) for j in range(inner)]
    fed = (ref != ref_small).any(0).any(0)
    sl.append(("columns fed by the large element of the last K chunk", (slice(None), slice(None), fed)))
    return sl


def _compare(what, got, ref, slices, tol):
    for name, idx in slices:
        a, b = got[idx], ref[idx]
        if b.numel() == 0:
            continue
        err = rel_l2(a, b)
        print(f"  {what} {name}: rel L2 {err:.3e} (bound {tol:g})")
        assert err < tol, (what, name, err, tol)


def _run(ops, dev, row, t):
    """The call of ``row``: the output (host), with checks b and c."""
    L = ops.L
    off = 0 if row.align == 16 else 1
    d = X.desc(L, row)
    info = X.instance_info(L, row)
    st = L.stream()
    g = {n: carve(v.to(dev), off) for n, v in t.items()}
    w16 = t["w"].to(dev)
    packed = [None, None]      # (the other direction's operand is not packed: a strided dilated conv has no data gradient here)
    packed[row.which] = torch.empty(L.lib.rh_conv1d_packed_floats(C.byref(d), row.which), device=dev)
    L.check(L.lib.rh_conv1d_pack_f32(C.byref(d), L.ptr(w16), L.ptr(packed[0]), L.ptr(packed[1]), st), "pack")
    wp = carve(packed[row.which], off)
    out = carve(torch.zeros(_out_shape(row), device=dev), off)
    nbytes = X.workspace_bytes(L, row) if row.ws else 0
    ws = carve(torch.zeros(nbytes // 4, device=dev), off) if nbytes > 0 else None
    L.lib.rh_x6_set_ranges(None, None, None, None)                                  # no slot armed
    if row.which == 0:
        rc = L.lib.rh_conv1d_fwd_f32(C.byref(d), L.ptr(g["x"]), L.ptr(wp), L.ptr(g.get("b")), L.ptr(g.get("alpha")), L.ptr(g.get("add")),
                                     L.ptr(out), L.ptr(ws), nbytes, st)
    else:
        rc = L.lib.rh_conv1d_bwd_data_f32(C.byref(d), L.ptr(g["dy"]), L.ptr(wp), L.ptr(g["x"]), L.ptr(g.get("alpha")), L.ptr(g.get("add")),
                                          L.ptr(out), L.ptr(ws), nbytes, st)
    L.check(rc, row.name)
    torch.cuda.synchronize()
    assert guards_intact(out), "guard words around the output were written"
    if ws is not None:
        assert guards_intact(ws), "the workspace was written beyond rh_conv1d_*_workspace_bytes"
    if info.ks > 1:
        assert ws is not None and bool((ws != 0).any()), "planned split in K, but no partial sum reached the workspace"
    elif ws is not None:
        assert not bool((ws != 0).any()), "an unsplit launch wrote into the workspace"
    if row.key.kmode == "nows":
        assert ws is None
    assert torch.isfinite(out).all()
    return out.cpu()


def _out_shape(row):
    g = X.gemm(row)
    return (g["B"], g["M"], g["out_row"])


@pytest.mark.parametrize("row", X.ROWS, ids=[r.name for r in X.ROWS])
def test_row(ops, dev, row):
    L = ops.L
    key = X.derive_key(L, row)
    assert key == row.key, (X.fmt_key(key), X.fmt_key(row.key))
    info = X.instance_info(L, row)
    t = _operands(row)
    ref, ref_small = _reference(row, t), _reference(row, t, big=False)
    assert tuple(ref.shape) == _out_shape(row)
    assert float(ref.norm()) / math.sqrt(ref.numel()) > 0.1                   # no output near zero in norm
    got = _run(ops, dev, row, t)
    print(f"{row.name}: {X.fmt_key(row.key)}")
    _compare("vs f64", got, ref, _slices(row, info, ref, ref_small), TOL_OP)
    # d. the 4-byte-aligned twin of a VEC row runs the element-wise variant: same bits when the plans agree
    if row.key.vec:
        twin = row._replace(align=4)
        ti = X.instance_info(L, twin)
        same = (ti.kernel, ti.ck, ti.ks, ti.TM, ti.TN, ti.WM, ti.WN) == (info.kernel, info.ck, info.ks, info.TM, info.TN, info.WM, info.WN)
        print(f"  twin at 4-byte alignment: vec {ti.vec}, ck {ti.ck} (row: {info.ck}), K slices {ti.ks} (row: {info.ks}) -> "
              f"{'bit identity asserted' if same else 'plans differ, not compared'}")
        assert not ti.vec
        if same:
            assert torch.equal(_run(ops, dev, twin._replace(key=row.key), t), got), "equal plans, different bits"

