"""Every row of the weight-gradient instance matrix (tests/wgrad_matrix.py) as direct ``rh_conv1d_bwd_weight_f32`` calls on
operands carved between guard words (tests/misaligned.py), checked:

a. against f64 on the CPU (torch.autograd.grad of F.conv1d / F.conv_transpose1d on the activated, padded f64 input, with respect to
   weight and bias), relative L2 below TOL_OP -- the tolerance of test_gpu_parity.py -- on the whole gradient AND on every slice
   (each tap, the last row and the last 32-row block, the last input channel, the last 32-column MFMA tile, the last workgroup column
   tile, the 32 columns either side of every workgroup-tile boundary, the bias gradient), so that a contribution missed at one tile
   edge or one tap is not averaged away;
b. family-1 rows against the f32-input kernels on the same operands (RH_WGRAD_X6=0, read per call), below the 2e-6 of
   test_gpu_wgrad_wide.py, on the same slices;
c. a second, EDGE-ISOLATING call of the same geometry whose R operand is zero except the last (partial) step of every batch item and
   the first max(pad_left, 1) / last max(pad_right, 1) positions: the whole gradient then comes from the tail and edge branches
   (Wx6RTasks::load: r_tail; wx6_step: s_edge; the pad offsets), same slices, same bounds;
d. the instance key is real on the device: guard words around dw, dbias and the workspace (offered at exactly
   rh_conv1d_workspace_bytes) intact; a row planned with Z > 1 has written partials into the zeroed workspace; a family-1 row of
   4096 gradient elements or more differs in bits from its family-0 result (the fallback is silent); two calls give the same bits;
   a wide-tile row gives the same bits under RH_WGRAD_X6_WIDE=2 and =0, a plane-staging row the same bits as RH_WGRAD_X6_PLANES=0
   under the same K slicing.
Both tolerances are the project's existing ones; nothing here is a new measurement.  tests/test_wgrad_matrix_host.py pins which
instance each row launches.  The deferred reduction and the weight-norm tail are compared bit for bit with the plain call at four
edge rows; tests/test_gpu_dispatch.py does the same through autograd at the workload's shapes.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import wgrad_matrix as W
from conftest import rel_l2
from misaligned import carve, guards_intact

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5       # tests/test_gpu_parity.py
TOL_F32 = 2e-6      # tests/test_gpu_wgrad_wide.py: x6 against the f32-input MFMA kernels
BIG = 40.0          # as in tests/test_gpu_x6_matrix.py: tests the range-slot scaling, reaches only the first and last steps


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    W.assert_default_planner_env()
    return _ops


def _operands(row):
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    gen = torch.Generator().manual_seed(W.seed(row.name))
    t = dict(x=torch.randn(B, Ci, Lx, generator=gen), dy=torch.randn(B, Co, W.out_len(row.geo), generator=gen))
    for v in t.values():
        v[-1, -1, -1] = BIG
        v[0, 0, 0] = BIG
    if row.act == "S":
        t["alpha"] = torch.rand(Ci, generator=gen) + 0.5
    return t


def _edge_only(row, t):
    """The operands of the edge-isolating call: R (dy; x for ConvTranspose1d) zeroed outside the last step of every batch item and
    the first max(pad_left, 1) / last max(pad_right, 1) positions."""
    pad = row.geo[7]
    which = "x" if row.geo[8] else "dy"
    r = t[which]
    n = r.shape[-1]
    keep = torch.zeros(n, dtype=torch.bool)
    keep[32 * (-(-n // 32) - 1):] = True
    keep[:max(pad[0], 1)] = True
    keep[n - max(pad[1], 1):] = True
    return dict(t, **{which: r * keep})


def _reference(row, t):
    """f64 on the CPU: (dw, dbias)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    x = t["x"].double()
    if row.act == "L":
        x = F.leaky_relu(x, W.SLOPE)
    elif row.act == "S":
        a = t["alpha"].double().view(1, -1, 1)
        x = x + torch.sin(a * x) ** 2 / (a + 1e-9)
    w = torch.zeros((Ci, Co, k) if tr else (Co, Ci, k), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose1d(x, w, b, stride=s, padding=pad[0]) if tr else F.conv1d(F.pad(x, pad), w, b, stride=s, dilation=dil)
    assert y.shape == t["dy"].shape
    dw, db = torch.autograd.grad(y, (w, b), t["dy"].double())
    return dw, db


def _slices(dw, db, cols):
    """{name: tensor} of the slices of a weight gradient [M][C][T] whose workgroup tiles are ``cols`` columns wide."""
    M, Cc, T = dw.shape
    N = Cc * T
    flat = dw.reshape(M, N)
    sl = {"whole": dw, "last row": dw[M - 1], "last 32-row block": dw[(M - 1) // 32 * 32:], "last input channel": dw[:, Cc - 1],
          "last 32-column tile": flat[:, (N - 1) // 32 * 32:], "last workgroup column tile": flat[:, (N - 1) // cols * cols:]}
    for t in range(T):
        sl[f"tap {t}"] = dw[..., t]
    for b in range(cols, N, cols):
        sl[f"columns around the tile boundary {b}"] = flat[:, b - 32:min(b + 32, N)]
    if db is not None:
        sl["bias gradient"] = db
    return sl


def _compare(what, got, ref, tol, worst):
    for name, b in ref.items():
        a = got[name]
        assert float(b.double().norm()) / math.sqrt(b.numel()) > 0.1, (what, name, "the reference slice is near zero")
        err = rel_l2(a, b)
        worst[what] = max(worst.get(what, (0.0, ""))[:2], (err, name))
        print(f"  {what} {name}: rel L2 {err:.3e} (bound {tol:g})")
        assert err < tol, (what, name, err, tol)


class _Call:
    """One row's calls: device operands at the row's pointer offset, range slots, and outputs / workspace between guard words."""

    def __init__(self, ops, dev, row):
        self.ops, self.L, self.dev, self.row = ops, ops.L, dev, row
        self.d = W.desc(self.L, row)
        B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
        self.wshape = (Ci, Co, k) if tr else (Co, Ci, k)
        self.Co = Co

    def load(self, t):
        L, dev = self.L, self.dev
        self.dy, self.x = carve(t["dy"].to(dev), self.row.off // 4), carve(t["x"].to(dev), self.row.off // 4)
        self.alpha = t["alpha"].to(dev) if "alpha" in t else None
        self.slots = []
        for v in (self.dy, self.x):
            slot = torch.zeros(self.ops._RANGE_WORDS, device=dev, dtype=torch.int32)
            L.check(L.lib.rh_amax_f32(L.ptr(v), v.numel(), L.ptr(slot), L.stream()), "amax")
            self.slots.append(slot)

    def arm(self):
        if self.row.armed:
            self.L.lib.rh_x6_set_ranges(self.L.ptr(self.slots[0]), self.L.ptr(self.slots[1]), None, None)
        else:
            self.L.lib.rh_x6_set_ranges(None, None, None, None)

    def buffers(self, **env):
        nbytes = W.workspace_bytes(self.L, self.row, **env)
        assert nbytes >= 0 and nbytes % 4 == 0
        nan = float("nan")
        self.dw = carve(torch.full(self.wshape, nan, device=self.dev), 0)
        self.db = carve(torch.full((self.Co,), nan, device=self.dev), 0) if self.row.bias else None
        self.ws = carve(torch.zeros(nbytes // 4, device=self.dev), 0) if nbytes else None
        self.nbytes = nbytes

    def check_buffers(self, info):
        torch.cuda.synchronize()
        assert guards_intact(self.dw), "guard words around dw were written"
        assert self.db is None or guards_intact(self.db), "guard words around dbias were written"
        if self.ws is not None:
            assert guards_intact(self.ws), "the workspace was written beyond rh_conv1d_workspace_bytes"
        if W.slicing(info)["Z"] > 1:
            bias_words = 64 * self.Co                                       # (the bias scratch comes first: rh_bias_grad_workspace)
            assert self.ws is not None and bool((self.ws[bias_words:] != 0).any()), "planned with Z > 1, but no partial sum reached the workspace"

    def run(self, **env):
        """The plain call under the row's switches plus ``env``: (dw, dbias) on the host, checked for guards and partials."""
        L = self.L
        info = W.instance_info(L, self.row, **env)
        self.buffers(**env)
        self.arm()
        with W.call_env(self.row, **env):
            rc = L.lib.rh_conv1d_bwd_weight_f32(C.byref(self.d), L.ptr(self.dy), L.ptr(self.x), L.ptr(self.alpha), L.ptr(self.dw), L.ptr(self.db),
                                                L.ptr(self.ws), self.nbytes, L.stream())
        L.check(rc, self.row.name)
        self.check_buffers(info)
        assert guards_intact(self.dy) and guards_intact(self.x)
        dw, db = self.dw.cpu(), None if self.db is None else self.db.cpu()
        assert torch.isfinite(dw).all() and (db is None or torch.isfinite(db).all()), "an element of the gradient was not written"
        return dw, db


def _same_slicing(a, b):
    return W.slicing(a)["Z"] == W.slicing(b)["Z"] and W.slicing(a)["per_z"] == W.slicing(b)["per_z"]


@pytest.mark.parametrize("row", W.ROWS, ids=[r.name for r in W.ROWS])
def test_row(ops, dev, row):
    L = ops.L
    info = W.instance_info(L, row)
    assert W.key_of(info) == row.key, (W.fmt_key(W.key_of(info)), W.fmt_key(row.key))
    print(f"{row.name}: {W.fmt_key(row.key)}")
    cols = W.slicing(info)["cols"]
    call = _Call(ops, dev, row)
    worst = {}
    full = _operands(row)
    for what, t in (("full", full), ("edge-only", _edge_only(row, full))):
        rdw, rdb = _reference(row, t)
        ref = _slices(rdw, rdb if row.bias else None, cols)
        call.load(t)
        dw, db = call.run()
        got = _slices(dw, db, cols)
        _compare(f"{what} vs f64", got, ref, TOL_OP, worst)
        dw2, db2 = call.run()
        assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), "two calls of one row differ in bits"
        if info[0] == 1 or not row.armed:
            off = W.instance_info(L, row, RH_WGRAD_X6=0)
            assert off[0] == 0
            dwf, dbf = call.run(RH_WGRAD_X6=0)
            if info[0] == 1:
                _compare(f"{what} vs family 0", got, _slices(dwf, dbf, cols), TOL_F32, worst)
                if dw.numel() >= 4096:
                    assert not torch.equal(dw, dwf), "the x6 result equals the f32-input result bit for bit: the fallback ran"
            else:       # no range slots: the same f32-input launch as with the x6 path switched off
                assert W.key_of(off) == row.key and torch.equal(dw, dwf) and (db is None or torch.equal(db, dbf))
        if info[0] == 1 and info[1]:                        # the wide tile with the 4-wave plan's K slicing == the 4-wave kernel
            i2, i0 = W.instance_info(L, row, RH_WGRAD_X6_WIDE=2), W.instance_info(L, row, RH_WGRAD_X6_WIDE=0)
            assert i2[1] == 1 and i0[1] == 0 and _same_slicing(i2, i0), (i2, i0)
            dww, dbw = call.run(RH_WGRAD_X6_WIDE=2)
            dw4, db4 = call.run(RH_WGRAD_X6_WIDE=0)
            assert torch.equal(dww, dw4) and (db is None or torch.equal(dbw, db4)), "wide tile != 4-wave tile under the same K slicing"
        if info[0] == 1 and info[6]:                        # plane staging == per-column staging under the same K slicing
            ip = W.instance_info(L, row, RH_WGRAD_X6_PLANES=0)
            assert ip[0] == 1 and ip[6] == 0
            base = dict(RH_WGRAD_X6_WIDE=2) if info[1] else {}
            assert _same_slicing(W.instance_info(L, row, **base), ip)
            dwp, dbp = call.run(**base)
            dwc, dbc = call.run(RH_WGRAD_X6_PLANES=0)
            assert torch.equal(dwp, dwc) and (db is None or torch.equal(dbp, dbc)), "plane staging != per-column staging"
    print("  worst: " + "; ".join(f"{k} {v[0]:.3e} ({v[1]})" for k, v in sorted(worst.items())))


TAIL_ROWS = ("wide tile, split", "4-wave tile, split", "unsplit")


def _tail_row(L, which):
    """Edge rows (a ragged last step) for the two other ways a call ends: family 1, N % 4 == 0 (the one-launch weight-norm form
    takes no other), with a K split on either tile and without one."""
    for r in W.ROWS:
        info = W.instance_info(L, r)
        if info[0] == 1 and W.gemm(r.geo)["N"] % 4 == 0 and W.edges(r, info) & {"r_row % 32 != 0, r_row % 4 == 0", "r_row % 4 != 0"}:
            if which == ("unsplit" if info[7] == 1 else ("wide tile, split" if info[1] else "4-wave tile, split")):
                return r
    raise AssertionError(f"no row for {which}")


@pytest.mark.parametrize("which", TAIL_ROWS)
def test_deferred_reduction_equals_the_plain_call(ops, dev, which):
    L = ops.L
    row = _tail_row(L, which)
    info = W.instance_info(L, row)
    call = _Call(ops, dev, row)
    call.load(_operands(row))
    dw, db = call.run()
    call.buffers()
    item = L.ReduceItem()
    L.check(L.lib.rh_defer_reduce(C.byref(item)), "defer")
    call.arm()
    with W.call_env(row):
        L.check(L.lib.rh_conv1d_bwd_weight_f32(C.byref(call.d), L.ptr(call.dy), L.ptr(call.x), None, L.ptr(call.dw), L.ptr(call.db),
                                               L.ptr(call.ws), call.nbytes, L.stream()), row.name)
    if info[7] > 1:
        assert (item.Z, item.n, item.out) == (info[7], dw.numel(), call.dw.data_ptr())
        L.check(L.lib.rh_reduce_partials_batched_f32(C.byref(item), 1, L.stream()), "batched reduce")
    else:
        assert item.Z == 0
    call.check_buffers(info)
    assert torch.equal(call.dw.cpu(), dw) and (db is None or torch.equal(call.db.cpu(), db))


@pytest.mark.parametrize("which", TAIL_ROWS)
def test_weight_norm_tail_equals_the_plain_call_and_f64(ops, dev, which):
    L = ops.L
    row = _tail_row(L, which)
    info = W.instance_info(L, row)
    call = _Call(ops, dev, row)
    t = _operands(row)
    call.load(t)
    dw, db = call.run()
    M, N = call.wshape[0], call.wshape[1] * call.wshape[2]
    gen = torch.Generator().manual_seed(W.seed(row.name) + 1)
    v = torch.randn(call.wshape, generator=gen).to(dev)
    g = (torch.rand(M, generator=gen) + 0.5).to(dev)
    norms = v.reshape(M, N).norm(dim=1).contiguous()
    dv0, dg0 = torch.empty_like(v), torch.empty_like(g)
    L.check(L.lib.rh_weight_norm_bwd_f32(L.ptr(call.dw), L.ptr(v), L.ptr(g), L.ptr(norms), M, N, L.ptr(dv0), L.ptr(dg0), L.stream()), "wn bwd")
    torch.cuda.synchronize()
    # f64 weight-norm backward of the f64 gradient
    dw64 = _reference(row, t)[0].reshape(M, N)
    v64, g64, n64 = v.cpu().double().reshape(M, N), g.cpu().double(), norms.cpu().double()
    dot = (dw64 * v64).sum(1)
    dg64 = dot / n64
    dv64 = (g64 / n64).unsqueeze(1) * (dw64 - v64 * (dot / n64 ** 2).unsqueeze(1))
    assert rel_l2(dv0.cpu().reshape(M, N), dv64) < TOL_OP and rel_l2(dg0.cpu(), dg64) < TOL_OP
    for fused in (0, 1):
        n0 = L.lib.rh_conv1d_bwd_weight_wn_fused_launches()
        call.buffers()
        dv = carve(torch.full(call.wshape, float("nan"), device=dev), 0)
        dg = carve(torch.full((M,), float("nan"), device=dev), 0)
        call.arm()
        with W.call_env(row), W.Env(dict(RH_WN_FUSED=fused)):
            L.check(L.lib.rh_conv1d_bwd_weight_wn_f32(C.byref(call.d), L.ptr(call.dy), L.ptr(call.x), None, L.ptr(v), L.ptr(g), L.ptr(norms),
                                                      L.ptr(call.dw), L.ptr(dv), L.ptr(dg), L.ptr(call.db), L.ptr(call.ws), call.nbytes,
                                                      L.stream()), row.name)
        call.check_buffers(info)
        assert guards_intact(dv) and guards_intact(dg)
        assert L.lib.rh_conv1d_bwd_weight_wn_fused_launches() == n0 + int(fused == 1 and info[7] > 1), "which form ran"
        assert torch.equal(dv, dv0) and torch.equal(dg, dg0), (fused, rel_l2(dv, dv0), rel_l2(dg, dg0))
        assert db is None or torch.equal(call.db.cpu(), db)
