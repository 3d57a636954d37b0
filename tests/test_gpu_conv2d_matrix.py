"""Every row of the 2-D convolution instance matrix (tests/conv2d_matrix.py) as one direct ``rh_conv2d_fwd_f32`` /
``rh_conv2d_bwd_data_f32`` / ``rh_conv2d_bwd_weight_f32`` call on operands carved between guard words (tests/misaligned.py), checked:

a. against f64 on the CPU (F.conv2d and its autograd), relative L2 below TOL_OP -- the tolerance of test_gpu_parity.py -- on the whole
   tensor AND on every edge slice (last batch item, last 32-row block, last row tile, last column tile, the padded border rows and
   columns, every output phase of a strided data gradient; for a weight gradient the first and last tap row and tap column, the last
   channel group, the last output channel, the bias gradient), so that an error confined to one tile edge is not averaged away; a
   slice whose reference is identically zero (a data-gradient phase without taps) must be zero bit for bit.  LeakyReLU outputs take
   their gates from the HIP output, as test_conv2d_fwd_and_grads_vs_cpu does; the fused-derivative rows get y with |y| > 0.1;
b. a second, EDGE-ISOLATING call of the same geometry whose input operand (x of a forward, dy of a gradient) is zero except in the
   last row tile, the last column tile and the first / last max(pad, 1) rows and columns: same slices, same bounds;
c. family-1 rows against the f32-input kernels on the same operands (RH_CONV2D_X6=0 / RH_WGRAD2D_X6=0, read per call), below the 2e-6
   of test_gpu_dispatch.py, on the same slices; a row of 4096 outputs or more differs in bits (the fallback is silent);
d. guard words around the output, dbias and the workspace (offered at exactly the row's bytes) intact; a weight gradient planned with
   Z > 1 has written partials into the zeroed workspace, one with Z == 1 has not; the published output range of a conv2d_x6_kernel
   row covers max |out|; two calls of a gradient row give the same bits.
Both tolerances are the project's existing ones.  tests/test_conv2d_matrix_host.py pins which instance each row launches.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import conv2d_matrix as M
from conftest import rel_l2
from misaligned import carve, guards_intact

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5       # tests/test_gpu_parity.py
TOL_SHADOW = 2e-6   # tests/test_gpu_dispatch.py: x6 against the f32-input MFMA kernels, per launch
BIG = 40.0          # as in tests/test_gpu_x6_matrix.py: tests the range-slot scaling
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    M.assert_default_planner_env()
    yield _ops
    for k, v in sorted(WORST.items()):
        print(f"largest rel L2, {k}: {v[0]:.3e} ({v[1]})")


def operands(row):
    """Host operands of a row: randn, the weights scaled so that no output is small in norm, one large element at the last position
    of the last batch item; y of a fused-derivative row with |y| > 0.1 (no gate can flip)."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    ho, wo = M.out_hw(row.geo)
    gen = torch.Generator().manual_seed(M.seed(row.name))
    fan = Ci * k[0] * k[1] if row.which == 0 else max(1.0, Co * k[0] * k[1] / (s[0] * s[1]))
    t = dict(x=torch.randn(B, Ci, H, W, generator=gen), w=torch.randn(Co, Ci, *k, generator=gen) * (2.0 / math.sqrt(fan)),
             b=torch.randn(Co, generator=gen), dy=torch.randn(B, Co, ho, wo, generator=gen))
    t["x"][-1, -1, -1, -1] = BIG
    t["dy"][-1, -1, -1, -1] = BIG
    sign = torch.where(torch.rand(B, Co, ho, wo, generator=gen) < 0.5, -1.0, 1.0)
    t["y"] = sign * (0.1 + 0.01 + torch.rand(B, Co, ho, wo, generator=gen))
    return t


def edge_only(row, info, t):
    """The operands of the edge-isolating call: the input operand of the kernel zeroed outside its last row tile, its last column tile
    and its first / last max(pad, 1) rows and columns."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    which = "x" if row.which == 0 else "dy"
    r = t[which]
    n_h, n_w = r.shape[-2:]
    TR, TQ = info[5], info[6]
    # first operand row / column that the last tile of the OUTPUT grid can read (forward: r0 * stride - pad; a gradient walks dy itself,
    # less the reach of the taps for a data gradient)
    if row.which == 0:
        h0 = ((M.out_hw(row.geo)[0] - 1) // TR * TR) * s[0] - pad[0]
        w0 = ((M.out_hw(row.geo)[1] - 1) // TQ * TQ) * s[1] - pad[1]
    elif row.which == 1:
        h0 = ((-(-H // s[0]) - 1) // TR * TR) - ((k[0] - 1) * dil[0]) // s[0] - 1
        w0 = ((-(-W // s[1]) - 1) // TQ * TQ) - ((k[1] - 1) * dil[1]) // s[1] - 1
    else:
        h0, w0 = (n_h - 1) // TR * TR, (n_w - 1) // TQ * TQ
    kh, kw = torch.zeros(n_h, dtype=torch.bool), torch.zeros(n_w, dtype=torch.bool)
    kh[max(0, min(h0, n_h - 1)):] = True
    kw[max(0, min(w0, n_w - 1)):] = True
    for keep, p in ((kh, pad[0]), (kw, pad[1])):
        keep[:max(p, 1)] = True
        keep[len(keep) - max(p, 1):] = True
    return dict(t, **{which: r * (kh.view(-1, 1) | kw.view(1, -1))})


def reference(row, t, gates=None):
    """f64 on the CPU.  Forward: y (LeakyReLU gates from ``gates``, the HIP output); data gradient: dx; weight gradient: (dw, dbias)."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    x, w, b = t["x"].double(), t["w"].double(), t["b"].double()
    if row.which == 0:
        y = F.conv2d(x, w, b if row.bias else None, s, pad, dil)
        return torch.where(gates > 0, y, M.SLOPE * y) if row.act else y
    cot = t["dy"].double()
    if row.act:       # the fused derivative: the activation-free gradient of dy * act'(y)
        cot = cot * torch.where(t["y"] > 0, 1.0, M.SLOPE).double()
    if row.which == 1:
        x0 = torch.zeros_like(x, requires_grad=True)
        (dx,) = torch.autograd.grad(F.conv2d(x0, w, None, s, pad, dil), x0, cot)
        return dx
    w0 = torch.zeros_like(w, requires_grad=True)
    b0 = torch.zeros_like(b, requires_grad=True)
    dw, db = torch.autograd.grad(F.conv2d(x, w0, b0, s, pad, dil), (w0, b0), cot)
    return dw, db


def slices(row, info, out):
    """{name: tensor} of the edge slices of an output: (B, M, h, w) of a convolution, (dw, dbias) of a weight gradient."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    TR, TQ = info[5], info[6]
    if row.which == 2:
        dw, db = out
        sl = {"whole": dw, "last output channel": dw[Co - 1], "last channel group": dw[:, (Ci - 1) // 32 * 32:],
              "first tap row": dw[:, :, 0], "last tap row": dw[:, :, -1], "first tap column": dw[..., 0], "last tap column": dw[..., -1]}
        if row.bias:
            sl["bias gradient"] = db
        return sl
    Bn, Mr, h, w = out.shape
    os_ = s if row.which == 1 else (1, 1)
    rows, qcols = -(-h // os_[0]), -(-w // os_[1])
    sl = {"whole": out, "last batch item": out[Bn - 1], "last 32-row block": out[:, (Mr - 1) // 32 * 32:],
          "last row tile": out[:, :, min((rows - 1) // TR * TR * os_[0], h - 1):], "last column tile": out[..., min((qcols - 1) // TQ * TQ * os_[1], w - 1):]}
    nh = (pad[0] if row.which == 1 else -(-pad[0] // s[0]))
    nw = (pad[1] if row.which == 1 else -(-pad[1] // s[1]))
    if nh:
        sl["first padded rows"], sl["last padded rows"] = out[:, :, :nh], out[:, :, max(0, h - nh):]
    if nw:
        sl["first padded columns"], sl["last padded columns"] = out[..., :nw], out[..., max(0, w - nw):]
    if row.which == 1 and s != (1, 1):
        for ah in range(min(s[0], h)):
            for aw in range(min(s[1], w)):
                sl[f"output phase ({ah}, {aw})"] = out[:, :, ah::s[0], aw::s[1]]
    return sl


def compare(what, got, ref, tol, floor, kind):
    for name, b in ref.items():
        a = got[name]
        if b.numel() == 0:
            continue
        if float(b.double().abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, (what, name, "the reference slice is zero, the result is not")
            continue
        if floor:
            assert float(b.double().norm()) / math.sqrt(b.numel()) > 0.1, (what, name, "the reference slice is near zero")
        err = rel_l2(a, b)
        k = f"{kind} {what.split(' vs ')[1]}"
        WORST[k] = max(WORST.get(k, (0.0, "")), (err, name))
        print(f"  {what} {name}: rel L2 {err:.3e} (bound {tol:g})")
        assert err < tol, (what, name, err, tol)


class _Call:
    """One row's calls: device operands at the row's pointer offset, range slots, and outputs / workspace between guard words."""

    def __init__(self, ops, dev, row):
        self.ops, self.L, self.dev, self.row = ops, ops.L, dev, row
        self.d = M.desc(self.L, row)
        B, Ci, Co, H, W, k, s, dil, pad = row.geo
        self.out_shape = ((B, Co) + M.out_hw(row.geo), (B, Ci, H, W), (Co, Ci) + tuple(k))[row.which]
        self.Co = Co

    def load(self, t):
        L, dev, row, o = self.L, self.dev, self.row, self.row.off // 4
        self.x, self.dy, self.y = carve(t["x"].to(dev), o), carve(t["dy"].to(dev), o), carve(t["y"].to(dev), o)
        self.b = t["b"].to(dev) if row.bias and row.which == 0 else None
        w = t["w"].to(dev)
        self.wp = [torch.empty(L.lib.rh_conv2d_packed_floats(C.byref(self.d), i), device=dev) for i in (0, 1)]
        L.check(L.lib.rh_conv2d_pack_f32(C.byref(self.d), L.ptr(w), L.ptr(self.wp[0]), L.ptr(self.wp[1]), L.stream()), "pack")
        self.slots = {}
        for n in ("x", "dy"):
            v = getattr(self, n)
            slot = torch.zeros(self.ops._RANGE_WORDS, device=dev, dtype=torch.int32)
            L.check(L.lib.rh_amax_f32(L.ptr(v), v.numel(), L.ptr(slot), L.stream()), "amax")
            self.slots[n] = slot

    def run(self, **env):
        """The call under the row's switches plus ``env``: the output on the host ((dw, dbias) for a weight gradient), checked for
        guards, workspace use and the published range."""
        L, row, dev = self.L, self.row, self.dev
        info = M.instance_info(L, row, **env)
        pl = M.plan(info, row.which)
        nan = float("nan")
        out = carve(torch.full(self.out_shape, nan, device=dev), 0)
        rout = torch.zeros(self.ops._RANGE_WORDS, device=dev, dtype=torch.int32)
        y = L.ptr(self.y) if row.act else None
        with M.call_env(row, **env):
            if row.which == 0:
                L.lib.rh_x6_set_ranges(None, L.ptr(self.slots["x"]) if row.armed else None, L.ptr(rout), None)
                rc = L.lib.rh_conv2d_fwd_f32(C.byref(self.d), L.ptr(self.x), L.ptr(self.wp[0]), L.ptr(self.b), L.ptr(out), L.stream())
            elif row.which == 1:
                L.lib.rh_x6_set_ranges(None, L.ptr(self.slots["dy"]) if row.armed else None, L.ptr(rout), None)
                rc = L.lib.rh_conv2d_bwd_data_f32(C.byref(self.d), L.ptr(self.dy), y, L.ptr(self.wp[1]), L.ptr(out), L.stream())
            else:
                nbytes = M.workspace_bytes(L, row)
                assert nbytes % 4 == 0
                db = carve(torch.full((self.Co,), nan, device=dev), 0) if row.bias else None
                ws = carve(torch.zeros(nbytes // 4, device=dev), 0) if nbytes else None
                if row.armed:
                    L.lib.rh_x6_set_ranges(L.ptr(self.slots["dy"]), L.ptr(self.slots["x"]), None, None)
                else:
                    L.lib.rh_x6_set_ranges(None, None, None, None)
                rc = L.lib.rh_conv2d_bwd_weight_f32(C.byref(self.d), L.ptr(self.dy), y, L.ptr(self.x), L.ptr(out), L.ptr(db), L.ptr(ws), nbytes,
                                                    L.stream())
        L.check(rc, row.name)
        torch.cuda.synchronize()
        assert guards_intact(out), "guard words around the output were written"
        assert guards_intact(self.x) and guards_intact(self.dy) and guards_intact(self.y)
        assert torch.isfinite(out).all(), "an element of the output was not written"
        if row.which < 2:
            assert float(rout.view(torch.float32).max()) >= float(out.abs().max()), "the published range does not cover the output"
            return out.cpu()
        assert db is None or (guards_intact(db) and torch.isfinite(db).all())
        if ws is not None:
            assert guards_intact(ws), "the workspace was written beyond the bytes offered"
            partials = ws[pl["bias_ws"] // 4:]
            if pl["Z"] > 1:
                assert bool((partials != 0).any()), "planned with Z > 1, but no partial sum reached the workspace"
            else:
                assert not bool((partials != 0).any()), "planned with Z == 1, but the workspace behind the bias scratch was written"
        else:
            assert pl["Z"] == 1
        return out.cpu(), None if db is None else db.cpu()


def _equal(a, b):
    if isinstance(a, tuple):
        return torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))
    return torch.equal(a, b)


@pytest.mark.parametrize("row", M.ROWS, ids=[r.name for r in M.ROWS])
def test_row(ops, dev, row):
    L = ops.L
    info = M.instance_info(L, row)
    assert M.key_of(info, row.which) == row.key, (M.fmt_key(M.key_of(info, row.which)), M.fmt_key(row.key))
    kind = M.kernel_of(info)
    print(f"{row.name}: {M.fmt_key(row.key)}")
    call = _Call(ops, dev, row)
    full = operands(row)
    for what, t in (("full", full), ("edge-only", edge_only(row, info, full))):
        call.load(t)
        got = call.run()
        ref = reference(row, t, gates=got if row.which == 0 else None)
        compare(f"{what} vs f64", slices(row, info, got), slices(row, info, ref), TOL_OP, what == "full", kind)
        if row.which > 0:
            assert _equal(got, call.run()), "two calls of one row differ in bits"
        if kind in ("x6", "wx6"):
            off = dict(RH_WGRAD2D_X6=0) if row.which == 2 else dict(RH_CONV2D_X6=0)
            assert M.kernel_of(M.instance_info(L, row, **off)) in ("dma", "igemm", "wdma", "wgrad", "smallm", "smallc")
            f0 = call.run(**off)
            compare(f"{what} vs family 0", slices(row, info, got), slices(row, info, f0), TOL_SHADOW, False, kind)
            main = got[0] if row.which == 2 else got
            if what == "full" and main.numel() >= 4096:
                assert not _equal(got, f0), "the x6 result equals the f32-input result bit for bit: the fallback ran"
