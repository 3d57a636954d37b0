"""The C ABI (include/rave_hip.h) at operands that are only 4-byte aligned, operand by operand, against f64 on the CPU.

The header promises "contiguous fp32, every pointer a device pointer owned by the caller" and asks nowhere for 16-byte
alignment; the host code selects a 16-byte vector path, an LDS-DMA staging path or another reduction kernel from
``(uintptr_t)ptr & 15`` at about twenty sites, and other kernels use 16-byte accesses justified by row lengths alone.  Every row
of the table below runs its entry point(s) through ctypes in seven arrangements: every operand aligned; every INPUT tensor carved
1, 2, 3 floats off a 16-byte boundary (tests/misaligned.py); every OUTPUT tensor carved likewise.  Tensors updated in place
count as both.  What stays aligned in every arrangement, because the header or the host code demands it: packed weights
(``wp_fwd`` / ``wp_bwd``: produced by the library's own pack kernels into buffers the caller sizes with
rh_conv1d_packed_floats), workspaces, range slots and the device scalars of rh_adam_step_f32.

Each arrangement is compared with an f64 evaluation of the operation on the CPU, under the tolerance the operator's existing
test uses (TOL_OP; rh_adam_step_f32: the bounds of test_fused_adam_kernel_matches_torch_adam).  Entry points without a direct
test of their own (``measured`` rows) may be at most twice as far from f64 as their own aligned arrangement -- the factor covers
another summation order only.  The guards of every carved tensor, inputs included, are compared bit for bit, and every carved
tensor asserts the residue it claims.

Covered: rh_weight_norm_{fwd,bwd,bwd_batched}, rh_reduce_partials_batched, rh_conv1d_{fwd,bwd_data,bwd_weight} (five
geometries, both kernel families), rh_residual_unit_fwd (and its refusal of misaligned packed weights, the only RH_ERR_* a
misaligned pointer draws), rh_conv2d_{fwd,bwd_data,bwd_weight} (four geometries, both RH_CONV2D_X6 values), the four direct PQMF
transforms, rh_amp_tanh_*, rh_act_fwd (Snake), rh_snake_bwd, rh_act_bwd, rh_act_bwd_bias, rh_adain_*, rh_avgpool2_*,
rh_pqmf_fold_k1 / _k2, rh_reparam_*, rh_stft_frame_{fwd,bwd,bwd_acc}, rh_spectral_distance_*, rh_stft_loss_{fwd,bwd} (n_fft 128 and
512), rh_feature_matching_*, rh_vq_ema_update, rh_adam_step in the table; rh_vq_assign_ws (bit-equality with the matrix-core
path) and rh_feed_batch_i16 / rh_feed_batch_pitch_i16 in tests of their own below.  rh_ema_update, rh_swap and rh_amax have
such tests elsewhere; rh_loss_combine_* works on scalars.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from misaligned import _Env, carve, guards_intact
from test_gpu_parity import TOL_OP


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


ARRANGEMENTS = [("aligned", 0)] + [(w, o) for w in ("inputs", "outputs") for o in (1, 2, 3)]


class Place:
    """Hands a row its device tensors in one arrangement and remembers the carved ones."""

    def __init__(self, dev, which, off):
        self.dev, self.which, self.off, self.carved = dev, which, off, []

    def _put(self, t, carved):
        if not carved:
            d = t.to(self.dev).contiguous()
            assert d.data_ptr() % 16 == 0
            return d
        off = self.off if t.element_size() <= 4 else 2        # int64 / double: the only misaligned residue they can take
        v = carve(t.to(self.dev), off)
        assert v.data_ptr() % 16 == 4 * off
        self.carved.append(v)
        return v

    def i(self, t):
        return self._put(t, self.which == "inputs")

    def o(self, *shape):
        return self._put(torch.full(shape, float("nan")), self.which == "outputs")

    def io(self, t):
        return self._put(t, self.which != "aligned")

    def aligned(self, t):
        return self._put(t, False)


def _lib():
    from rave_amd import _lib as L
    return L


def _s():
    return torch.cuda.current_stream().cuda_stream


_REF = {}


def _ref(key, fn):
    """The f64 reference of a row: computed once, shared by the seven arrangements, never modified."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ rows
def _wn_data(cols, seed):
    g = _gen(seed)
    return torch.randn(5, cols, generator=g), torch.rand(5, generator=g) + 0.5, torch.randn(5, cols, generator=g)


def _wn_ref(v, g, dw):
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    w = g64[:, None] * v64 / v64.norm(dim=1, keepdim=True)
    w.backward(dw.double())
    return dict(w=w.detach(), norms=v64.detach().norm(dim=1), dv=v64.grad, dg=g64.grad)


def row_weight_norm(P, cols):
    L = _lib()
    v, g, dw = _wn_data(cols, 100 + cols)
    want = _ref(("wn", cols), lambda: _wn_ref(v, g, dw))
    vd, gd, dwd = P.i(v), P.i(g), P.i(dw)
    w, norms, dv, dg = P.o(5, cols), P.o(5), P.o(5, cols), P.o(5)
    L.check(L.lib.rh_weight_norm_fwd_f32(L.ptr(vd), L.ptr(gd), 5, cols, L.ptr(w), L.ptr(norms), _s()), "weight_norm_fwd")
    # (norms is an output of the first call and an input of the second: it keeps the placement of an output)
    L.check(L.lib.rh_weight_norm_bwd_f32(L.ptr(dwd), L.ptr(vd), L.ptr(gd), L.ptr(norms), 5, cols, L.ptr(dv), L.ptr(dg), _s()),
            "weight_norm_bwd")
    return dict(w=w, norms=norms, dv=dv, dg=dg), want


def row_weight_norm_batched(P):
    """Three tensors (5 x 12, 5 x 13, 5 x 12) in one launch: the same bits as rh_weight_norm_bwd_f32 per tensor (header)."""
    L = _lib()
    got, want, keep = {}, {}, []
    arr = (L.WnBwdItem * 3)()
    singles = []
    for n, cols in enumerate((12, 13, 12)):
        v, g, dw = _wn_data(cols, 200 + n)
        ref = _ref(("wnb", n), lambda: _wn_ref(v, g, dw))
        vd, gd, dwd, nd = P.i(v), P.i(g), P.i(dw), P.i(ref["norms"].float())
        dv, dg = P.o(5, cols), P.o(5)
        a = arr[n]
        a.dw, a.v, a.g, a.norms, a.dv, a.dg, a.rows, a.cols = L.ptr(dwd), L.ptr(vd), L.ptr(gd), L.ptr(nd), L.ptr(dv), L.ptr(dg), 5, cols
        keep += [vd, gd, dwd, nd]
        got[f"dv{n}"], got[f"dg{n}"] = dv, dg
        want[f"dv{n}"], want[f"dg{n}"] = ref["dv"], ref["dg"]
        dv1, dg1 = torch.empty(5, cols, device=P.dev), torch.empty(5, device=P.dev)
        L.check(L.lib.rh_weight_norm_bwd_f32(L.ptr(dwd), L.ptr(vd), L.ptr(gd), L.ptr(nd), 5, cols, L.ptr(dv1), L.ptr(dg1), _s()), "wn_bwd")
        singles.append((dv, dv1, dg, dg1))
    L.check(L.lib.rh_weight_norm_bwd_batched_f32(arr, 3, _s()), "weight_norm_bwd_batched")
    torch.cuda.synchronize()
    for dv, dv1, dg, dg1 in singles:
        assert torch.equal(dv, dv1) and torch.equal(dg, dg1)
    return got, want


def row_reduce_partials(P, n, Z):
    """(65536, 4): aligned operands take the 16-byte kernel of reduce_is_vec4 (conv_wgrad.hip), a misaligned ``part`` or ``out``
    the 64-elements-per-workgroup kernel; (1001, 3) takes the latter always."""
    L = _lib()
    part = torch.randn(Z, n, generator=_gen(300 + Z))
    want = _ref(("red", n, Z), lambda: dict(out=part.double().sum(0)))
    pd, out = P.i(part), P.o(n)
    arr = (L.ReduceItem * 1)()
    arr[0].part, arr[0].out, arr[0].n, arr[0].Z = L.ptr(pd), L.ptr(out), n, Z
    L.check(L.lib.rh_reduce_partials_batched_f32(arr, 1, _s()), "reduce_partials_batched")
    return dict(out=out), want


CONVS = {
    # name: (c_in, c_out, L, k, stride, pad, transposed, act, bias, residual)          B = 2
    "c32_96_L64": (32, 96, 64, 3, 1, 1, False, 1, True, True),
    "c32_96_L66": (32, 96, 66, 3, 1, 1, False, 1, True, True),
    "first_layer_1_16": (1, 16, 300, 5, 4, 2, False, 0, True, False),
    "out_layer_96_32": (96, 32, 1028, 7, 1, 3, False, 1, True, False),
    "transposed_64_32": (64, 32, 9, 16, 8, 4, True, 1, True, False),
}


def _conv_data(name):
    c_in, c_out, Lin, k, stride, pad, tr, act, has_b, has_r = CONVS[name]
    g = _gen(400 + list(CONVS).index(name))
    from rave_amd.ops import ConvGeom
    geom = ConvGeom(stride=stride, pad_left=pad, pad_right=pad, transposed=tr, act=act, slope=0.2)
    l_out = geom.out_len(Lin, k)
    x = torch.randn(2, c_in, Lin, generator=g)
    w = torch.randn((c_in, c_out, k) if tr else (c_out, c_in, k), generator=g) / math.sqrt(c_in * k)
    b = torch.randn(c_out, generator=g) if has_b else None
    r = torch.randn(2, c_out, l_out, generator=g) if has_r else None
    cot = torch.randn(2, c_out, l_out, generator=g)
    return geom, l_out, x, w, b, r, cot


def _conv_ref(name):
    c_in, c_out, Lin, k, stride, pad, tr, act, has_b, has_r = CONVS[name]
    geom, l_out, x, w, b, r, cot = _conv_data(name)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if has_b else None
    xa = F.leaky_relu(x64, 0.2) if act == 1 else x64
    y = F.conv_transpose1d(xa, w64, b64, stride, pad) if tr else F.conv1d(xa, w64, b64, stride, pad)
    if has_r:
        y = y + r.double()
    assert y.shape[-1] == l_out
    y.backward(cot.double())
    return dict(y=y.detach(), dx=x64.grad, dw=w64.grad, db=None if b64 is None else b64.grad)


def row_conv1d(P, name, x6):
    """rh_conv1d_fwd_f32 / _bwd_data_f32 / _bwd_weight_f32 on one geometry.  ``x6``: range slots armed, i.e. the f16-piece
    matrix-core kernels where the geometry has them; otherwise RH_CONV_X6=0 RH_WGRAD_X6=0, the f32-input kernels (LDS-DMA
    staging, conv_igemm_dma.hip / conv_wgrad.hip)."""
    L = _lib()
    from rave_amd.ops import _desc
    c_in, c_out, Lin, k, stride, pad, tr, act, has_b, has_r = CONVS[name]
    geom, l_out, x, w, b, r, cot = _conv_data(name)
    want = _ref(("conv", name), lambda: _conv_ref(name))
    d = _desc(geom, 2, c_in, c_out, Lin, l_out, k)
    dref = C.byref(d)
    dev, s = P.dev, _s()
    words = L.lib.rh_x6_range_words()

    def slot(t):
        sl = torch.zeros(words, dtype=torch.int32, device=dev)
        L.check(L.lib.rh_amax_f32(L.ptr(t), t.numel(), L.ptr(sl), s), "amax")
        return sl

    def ws(nbytes):
        return torch.empty(max(int(nbytes), 16) // 4, device=dev), int(nbytes)

    with _Env(RH_CONV_X6=None if x6 else 0, RH_WGRAD_X6=None if x6 else 0, RH_WGRAD_X6_BLOCKS=None, RH_WGRAD_X6_WIDE=None,
              RH_WGRAD_X6_PLANES=None):
        wd = P.i(w)
        wp_f = torch.empty(L.lib.rh_conv1d_packed_floats(dref, 0), device=dev)          # packed operands: always aligned
        wp_b = torch.empty(L.lib.rh_conv1d_packed_floats(dref, 1), device=dev)
        L.check(L.lib.rh_conv1d_pack_f32(dref, L.ptr(wd), L.ptr(wp_f), L.ptr(wp_b), s), "pack")
        xd, cd = P.i(x), P.i(cot)
        bd = None if b is None else P.i(b)
        rd = None if r is None else P.i(r)
        y, dx, dw = P.o(*want["y"].shape), P.o(*x.shape), P.o(*w.shape)
        db = None if b is None else P.o(c_out)
        sx, sc = (slot(xd), slot(cd)) if x6 else (None, None)
        wsp, nb = ws(L.lib.rh_conv1d_fwd_workspace_bytes(dref))
        if x6:
            L.lib.rh_x6_set_ranges(None, L.ptr(sx), None, None)
        L.check(L.lib.rh_conv1d_fwd_f32(dref, L.ptr(xd), L.ptr(wp_f), L.ptr(bd), None, L.ptr(rd), L.ptr(y), L.ptr(wsp), nb, s), "fwd")
        wsp2, nb2 = ws(L.lib.rh_conv1d_bwd_data_workspace_bytes(dref))
        if x6:
            L.lib.rh_x6_set_ranges(None, L.ptr(sc), None, None)
        L.check(L.lib.rh_conv1d_bwd_data_f32(dref, L.ptr(cd), L.ptr(wp_b), L.ptr(xd), None, None, L.ptr(dx), L.ptr(wsp2), nb2, s), "dgrad")
        wsp3, nb3 = ws(L.lib.rh_conv1d_workspace_bytes(dref))
        if x6:
            L.lib.rh_x6_set_ranges(L.ptr(sc), L.ptr(sx), None, None)
        L.check(L.lib.rh_conv1d_bwd_weight_f32(dref, L.ptr(cd), L.ptr(xd), None, L.ptr(dw), L.ptr(db), L.ptr(wsp3), nb3, s), "wgrad")
        L.lib.rh_x6_set_ranges(None, None, None, None)
        torch.cuda.synchronize()
    got = dict(y=y, dx=dx, dw=dw)
    if db is not None:
        got["db"] = db
    return got, want


def _bcl(l, seed):
    g = _gen(seed)
    return torch.randn(2, 6, l, generator=g), torch.randn(2, 6, l, generator=g)


def row_amp_tanh(P, l):
    L = _lib()
    g = _gen(500 + l)
    x, dy = torch.randn(2, 12, l, generator=g), torch.randn(2, 6, l, generator=g)

    def ref():
        x64 = x.double().requires_grad_(True)
        y = torch.tanh(x64[:, :6] * torch.sigmoid(x64[:, 6:]))
        y.backward(dy.double())
        return dict(y=y.detach(), dx=x64.grad)
    want = _ref(("amp", l), ref)
    xd, dyd, y, dx = P.i(x), P.i(dy), P.o(2, 6, l), P.o(2, 12, l)
    L.check(L.lib.rh_amp_tanh_fwd_f32(L.ptr(xd), 2, 6, l, L.ptr(y), _s()), "amp_tanh_fwd")
    L.check(L.lib.rh_amp_tanh_bwd_f32(L.ptr(dyd), L.ptr(xd), 2, 6, l, L.ptr(dx), _s()), "amp_tanh_bwd")
    return dict(y=y, dx=dx), want


def row_snake(P, l):
    """rh_act_fwd_f32 (Snake) and rh_snake_bwd_f32: no direct test of their own (measured row)."""
    L = _lib()
    x, dy = _bcl(l, 600 + l)
    alpha = torch.rand(6, generator=_gen(601)) + 0.5

    def ref():
        x64, a64 = x.double().requires_grad_(True), alpha.double().requires_grad_(True)
        a = a64[None, :, None]
        y = x64 + (a + 1e-9).reciprocal() * (a * x64).sin().pow(2)
        y.backward(dy.double())
        return dict(y=y.detach(), dx=x64.grad, dalpha=a64.grad)
    want = _ref(("snake", l), ref)
    xd, dyd, ad = P.i(x), P.i(dy), P.i(alpha)
    y, dx, da = P.o(2, 6, l), P.o(2, 6, l), P.o(6)
    L.check(L.lib.rh_act_fwd_f32(L.ptr(xd), L.ptr(ad), 2, 0.0, 2, 6, l, L.ptr(y), _s()), "act_fwd")
    nb = L.lib.rh_snake_bwd_workspace_bytes(2, 6)
    ws = torch.empty(max(nb, 16) // 4, device=P.dev)
    L.check(L.lib.rh_snake_bwd_f32(L.ptr(dyd), L.ptr(xd), L.ptr(ad), 2, 6, l, L.ptr(dx), L.ptr(da), L.ptr(ws), nb, _s()), "snake_bwd")
    return dict(y=y, dx=dx, dalpha=da), want


def row_act_bwd(P, l):
    """rh_act_bwd_f32 and rh_act_bwd_bias_f32 (output LeakyReLU 0.1): g = dy * act'(y), dbias = sum g."""
    L = _lib()
    yv, dy = _bcl(l, 700 + l)

    def ref():
        g = dy.double() * torch.where(yv.double() >= 0, 1.0, 0.1)
        return dict(g=g, g2=g, dbias=g.sum((0, 2)))
    want = _ref(("actb", l), ref)
    yd, dyd = P.i(yv), P.i(dy)
    g, g2, db = P.o(2, 6, l), P.o(2, 6, l), P.o(6)
    L.check(L.lib.rh_act_bwd_f32(L.ptr(dyd), L.ptr(yd), 1, 0.1, 2 * 6 * l, L.ptr(g), _s()), "act_bwd")
    nb = L.lib.rh_act_bwd_bias_workspace_bytes(6)
    ws = torch.empty(max(nb, 16) // 4, device=P.dev)
    L.check(L.lib.rh_act_bwd_bias_f32(L.ptr(dyd), L.ptr(yd), 1, 0.1, 2, 6, l, L.ptr(g2), L.ptr(db), L.ptr(ws), nb, _s()), "act_bwd_bias")
    return dict(g=g, g2=g2, dbias=db), want


def row_avgpool2(P, l):
    L = _lib()
    g = _gen(800 + l)
    x, dy = torch.randn(12, l, generator=g), torch.randn(12, l // 2, generator=g)

    def ref():
        x64 = x.double().requires_grad_(True)
        y = F.avg_pool1d(x64[None], 2)[0]
        y.backward(dy.double())
        return dict(y=y.detach(), dx=x64.grad)
    want = _ref(("pool", l), ref)
    xd, dyd, y, dx = P.i(x), P.i(dy), P.o(12, l // 2), P.o(12, l)
    L.check(L.lib.rh_avgpool2_fwd_f32(L.ptr(xd), 12, l, L.ptr(y), _s()), "avgpool2_fwd")
    L.check(L.lib.rh_avgpool2_bwd_f32(L.ptr(dyd), 12, l, L.ptr(dx), _s()), "avgpool2_bwd")
    return dict(y=y, dx=dx), want


CONV2DS = {
    # name: (c_in, c_out, H, W, (kh, kw), stride, (ph, pw))          B = 2
    "c16_16_9x13_k3x3": (16, 16, 9, 13, (3, 3), 1, (1, 1)),
    "c3_5_7x6_k3x2_s2": (3, 5, 7, 6, (3, 2), 2, (1, 1)),
    "one_output_channel_16_1": (16, 1, 9, 13, (3, 3), 1, (1, 1)),        # conv2d_smallm.hip
    "small_c_2_8_33x13_k9x3": (2, 8, 33, 13, (9, 3), 1, (4, 1)),        # conv2d_smallc.hip
}


def _conv2d_data(name):
    c_in, c_out, H, W, k, st, pad = CONV2DS[name]
    g = _gen(900 + list(CONV2DS).index(name))
    x = torch.randn(2, c_in, H, W, generator=g)
    w = torch.randn(c_out, c_in, *k, generator=g) / math.sqrt(c_in * k[0] * k[1])
    b = torch.randn(c_out, generator=g)
    y = F.conv2d(x, w, b, st, pad)
    cot = torch.randn(y.shape, generator=g)
    return x, w, b, cot


def _conv2d_ref(name):
    c_in, c_out, H, W, k, st, pad = CONV2DS[name]
    x, w, b, cot = _conv2d_data(name)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    pre = F.conv2d(x64, w64, b64, st, pad)
    pre.backward(cot.double())
    return dict(y=F.leaky_relu(pre.detach(), 0.2), dx=x64.grad, dw=w64.grad, db=b64.grad)


def row_conv2d(P, name, x6):
    """rh_conv2d_fwd_f32 (with its output LeakyReLU) and, on the activation-free descriptor the backward of rave_amd.ops uses,
    rh_conv2d_bwd_data_f32 / rh_conv2d_bwd_weight_f32; ``x6`` = RH_CONV2D_X6 (1: f16-piece matrix-core kernels where the
    geometry has them, range slots armed as rave_amd.ops arms them; 0: conv2d.hip / conv2d_smallm.hip / conv2d_smallc.hip)."""
    L = _lib()
    c_in, c_out, H, W, k, st, pad = CONV2DS[name]
    x, w, b, cot = _conv2d_data(name)
    want = _ref(("conv2d", name), lambda: _conv2d_ref(name))
    dev, s = P.dev, _s()
    h_out, w_out = want["y"].shape[2:]
    words = L.lib.rh_x6_range_words()

    def desc(act):
        return L.Conv2dDesc(batch=2, c_in=c_in, c_out=c_out, h_in=H, w_in=W, h_out=h_out, w_out=w_out, kh=k[0], kw=k[1], sh=st, sw=st,
                            dh=1, dw=1, ph=pad[0], pw=pad[1], act=act, act_slope=0.2)

    def slot(t=None):
        sl = torch.zeros(words, dtype=torch.int32, device=dev)
        if t is not None:
            L.check(L.lib.rh_amax_f32(L.ptr(t), t.numel(), L.ptr(sl), s), "amax")
        return sl

    def family(d, which):
        info = (C.c_int64 * 16)()
        return int(info[0]) if L.lib.rh_conv2d_plan_info(C.byref(d), which, info) == 0 else 0

    with _Env(RH_CONV2D_X6=x6, RH_CONV_X6=None):
        d1, d0 = desc(1), desc(0)
        wd = P.i(w)
        wp_f = torch.empty(L.lib.rh_conv2d_packed_floats(C.byref(d1), 0), device=dev)      # packed operands: always aligned
        wp_b = torch.empty(L.lib.rh_conv2d_packed_floats(C.byref(d1), 1), device=dev)
        L.check(L.lib.rh_conv2d_pack_f32(C.byref(d1), L.ptr(wd), L.ptr(wp_f), L.ptr(wp_b), s), "conv2d_pack")
        xd, cd, bd = P.i(x), P.i(cot), P.i(b)
        y, dx, dw, db = P.o(*want["y"].shape), P.o(*x.shape), P.o(*w.shape), P.o(c_out)
        sx, sc = slot(xd), slot(cd)
        L.lib.rh_x6_set_ranges(None, L.ptr(sx) if family(d1, 0) == 1 else None, L.ptr(slot()), None)
        L.check(L.lib.rh_conv2d_fwd_f32(C.byref(d1), L.ptr(xd), L.ptr(wp_f), L.ptr(bd), L.ptr(y), s), "conv2d_fwd")
        L.lib.rh_x6_set_ranges(None, L.ptr(sc) if family(d0, 1) == 1 else None, L.ptr(slot()), None)
        L.check(L.lib.rh_conv2d_bwd_data_f32(C.byref(d0), L.ptr(cd), None, L.ptr(wp_b), L.ptr(dx), s), "conv2d_bwd_data")
        nb = int(L.lib.rh_conv2d_workspace_bytes(C.byref(d0)))
        ws = torch.empty(max(nb, 16) // 4, device=dev)
        if L.lib.rh_conv2d_bwd_weight_kernel_family(C.byref(d0)) == 1:
            L.lib.rh_x6_set_ranges(L.ptr(sc), L.ptr(sx), None, None)
        L.check(L.lib.rh_conv2d_bwd_weight_f32(C.byref(d0), L.ptr(cd), None, L.ptr(xd), L.ptr(dw), L.ptr(db), L.ptr(ws), nb, s),
                "conv2d_bwd_weight")
        L.lib.rh_x6_set_ranges(None, None, None, None)
        torch.cuda.synchronize()
    return dict(y=y, dx=dx, dw=dw, db=db), want


def _unit_setup(dev):
    """Residual(DilatedUnit) at C = 32, L = 64, B = 2 (k3 dilation 3, then 1x1; LeakyReLU 0.2 in front of both)."""
    L = _lib()
    from rave_amd.ops import ConvGeom, _desc
    g = _gen(950)
    x = torch.randn(2, 32, 64, generator=g)
    w3 = torch.randn(32, 32, 3, generator=g) / math.sqrt(96)
    w1 = torch.randn(32, 32, 1, generator=g) / math.sqrt(32)
    d3 = _desc(ConvGeom(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2), 2, 32, 32, 64, 64, 3)
    d1 = _desc(ConvGeom(act=1, slope=0.2), 2, 32, 32, 64, 64, 1)
    packed = []
    for d, w in ((d3, w3), (d1, w1)):
        wp = torch.empty(L.lib.rh_conv1d_packed_floats(C.byref(d), 0), device=dev)
        L.check(L.lib.rh_conv1d_pack_f32(C.byref(d), L.ptr(w.to(dev)), L.ptr(wp), None, _s()), "pack")
        packed.append(wp)
    return x, w3, w1, d3, d1, packed


def row_residual_unit(P):
    """rh_residual_unit_fwd_f32 with x, h, y carved; the packed weights stay aligned (unit_x6.hip refuses otherwise: the test
    below).  The input's range slot is armed, as the f16 kernel demands."""
    L = _lib()
    x, w3, w1, d3, d1, (wp3, wp1) = _unit_setup(P.dev)
    assert L.lib.rh_residual_unit_fused(C.byref(d3), C.byref(d1)) == 1

    def ref():
        x64 = x.double()
        h = F.conv1d(F.leaky_relu(x64, 0.2), w3.double(), None, 1, 3, 3)
        return dict(h=h, y=F.conv1d(F.leaky_relu(h, 0.2), w1.double()) + x64)
    want = _ref("unit", ref)
    xd, h, y = P.i(x), P.o(2, 32, 64), P.o(2, 32, 64)
    sl = torch.zeros(L.lib.rh_x6_range_words(), dtype=torch.int32, device=P.dev)
    L.check(L.lib.rh_amax_f32(L.ptr(xd), xd.numel(), L.ptr(sl), _s()), "amax")
    L.lib.rh_x6_set_ranges(None, L.ptr(sl), None, None)
    L.check(L.lib.rh_residual_unit_fwd_f32(C.byref(d3), C.byref(d1), L.ptr(xd), L.ptr(wp3), L.ptr(wp1), L.ptr(h), L.ptr(y), _s()), "unit")
    return dict(h=h, y=y), want


def row_pqmf(P, causal):
    """The four direct-form PQMF transforms, rows = 2, T = 1024 + 16 (pqmf.hip stores 16 bytes at a time, justified by the row
    length alone)."""
    import rave_oracle as O
    L = _lib()
    sd = O.pqmf_buffers(100, 16)
    wf, wi = sd["forward_conv.weight"], sd["inverse_conv.weight"]
    mode = "causal" if causal else "centered"
    T, K, K2 = 1040, wf.shape[-1], wi.shape[-1]
    pf, pi = O.get_padding(K, mode=mode), O.get_padding(K2, mode=mode)
    nfr = (T + pf[0] + pf[1] - K) // 16 + 1
    n_out = nfr + pi[0] + pi[1] - K2 + 1
    g = _gen(960 + int(causal))
    x = O.synthetic_batch(2, 1, T, seed=7)
    cy, yin, cx = torch.randn(2, 16, nfr, generator=g), torch.randn(2, 16, nfr, generator=g), torch.randn(2, 1, n_out * 16, generator=g)

    def ref():
        x64, y64 = x.double().requires_grad_(True), yin.double().requires_grad_(True)
        ya = O.pqmf_analysis(x64, wf.double(), causal)
        ya.backward(cy.double())
        xs = O.pqmf_synthesis(y64, wi.double(), causal)
        xs.backward(cx.double())
        assert ya.shape == (2, 16, nfr) and xs.shape == (2, 1, n_out * 16)
        return dict(y=ya.detach(), dx=x64.grad, xs=xs.detach(), dy=y64.grad)
    want = _ref(("pqmf", causal), ref)
    xd, cyd, yd, cxd, wfd, wid = P.i(x), P.i(cy), P.i(yin), P.i(cx), P.i(wf), P.i(wi)
    y, dx, xs, dy = P.o(2, 16, nfr), P.o(2, 1, T), P.o(2, 1, n_out * 16), P.o(2, 16, nfr)
    s = _s()
    L.check(L.lib.rh_pqmf_analysis_fwd_f32(L.ptr(xd), L.ptr(wfd), 2, T, 16, K, pf[0], nfr, L.ptr(y), s), "pqmf_analysis_fwd")
    L.check(L.lib.rh_pqmf_analysis_bwd_f32(L.ptr(cyd), L.ptr(wfd), 2, T, 16, K, pf[0], nfr, L.ptr(dx), s), "pqmf_analysis_bwd")
    L.check(L.lib.rh_pqmf_synthesis_fwd_f32(L.ptr(yd), L.ptr(wid), 2, nfr, 16, K2, pi[0], n_out, L.ptr(xs), s), "pqmf_synthesis_fwd")
    L.check(L.lib.rh_pqmf_synthesis_bwd_f32(L.ptr(cxd), L.ptr(wid), 2, nfr, 16, K2, pi[0], n_out, L.ptr(dy), s), "pqmf_synthesis_bwd")
    return dict(y=y, dx=dx, xs=xs, dy=dy), want


def row_adain(P, l):
    """rh_adain_stats_update_f32 (running statistics updated in place) and rh_adain_transfer_f32: measured row."""
    L = _lib()
    g = _gen(970 + l)
    x = torch.randn(12, l, generator=g) * 2 + 0.5
    mean0, std0 = torch.randn(12, generator=g), torch.rand(12, generator=g) + 0.5
    my, sy = torch.randn(12, generator=g), torch.rand(12, generator=g) + 0.5
    nup = torch.tensor([2.0])

    def ref():
        x64 = x.double()
        m = mean0.double() + (x64.mean(-1) - mean0.double()) / 3.0
        sd = std0.double() + (x64.std(-1) - std0.double()) / 3.0
        y = (x64 - mean0.double()[:, None]) / (std0.double()[:, None] + 1e-5) * sy.double()[:, None] + my.double()[:, None]
        return dict(mean=m, std=sd, y=y)
    want = _ref(("adain", l), ref)
    xd, nd = P.i(x), P.i(nup)
    mx, sx, myd, syd = P.i(mean0), P.i(std0), P.i(my), P.i(sy)
    mb, sb, y = P.io(mean0), P.io(std0), P.o(12, l)
    L.check(L.lib.rh_adain_stats_update_f32(L.ptr(xd), 12, l, L.ptr(nd), L.ptr(mb), L.ptr(sb), _s()), "adain_stats_update")
    L.check(L.lib.rh_adain_transfer_f32(L.ptr(xd), 12, l, L.ptr(mx), L.ptr(sx), L.ptr(myd), L.ptr(syd), L.ptr(y), _s()), "adain_transfer")
    return dict(mean=mb, std=sb, y=y), want


def row_reparam(P, l):
    import rave_oracle as O
    L = _lib()
    g = _gen(980 + l)
    z, eps, dzs = torch.randn(2, 12, l, generator=g), torch.randn(2, 6, l, generator=g), torch.randn(2, 6, l, generator=g)

    def ref():
        z64 = z.double().requires_grad_(True)
        zs, kl = O.reparametrize(z64, eps.double())
        torch.autograd.backward([zs, kl], [dzs.double(), torch.tensor(0.7, dtype=torch.float64)])
        return dict(zs=zs.detach(), kl=kl.detach().reshape(1), dz=z64.grad)
    want = _ref(("reparam", l), ref)
    zd, ed, dd, dk = P.i(z), P.i(eps), P.i(dzs), P.i(torch.tensor([0.7]))
    zs, kl, dz = P.o(2, 6, l), P.o(1), P.o(2, 12, l)
    nb = L.lib.rh_reparam_workspace_bytes()
    ws = torch.empty(max(nb, 16) // 4, device=P.dev)
    L.check(L.lib.rh_reparam_fwd_f32(L.ptr(zd), L.ptr(ed), 2, 6, l, L.ptr(zs), L.ptr(kl), L.ptr(ws), nb, _s()), "reparam_fwd")
    L.check(L.lib.rh_reparam_bwd_f32(L.ptr(zd), L.ptr(ed), L.ptr(dd), L.ptr(dk), 2, 6, l, L.ptr(dz), _s()), "reparam_bwd")
    return dict(zs=zs, kl=kl, dz=dz), want


def row_stft_frames(P):
    """rh_stft_frame_fwd_f32 / _bwd_f32 / _bwd_acc_f32, rows = 3, t = 1000, n_fft = 128, hop = 32 (misc.hip takes its 16-byte path
    from x | window | frames, resp. dframes | window | dx)."""
    L = _lib()
    rows, t, n, hop = 3, 1000, 128, 32
    nf = t // hop + 1
    g = _gen(990)
    x, dfr, base = torch.randn(rows, t, generator=g), torch.randn(rows, nf, n, generator=g), torch.randn(rows, t, generator=g)
    win = torch.hann_window(n)

    def ref():
        x64 = x.double().requires_grad_(True)
        xp = F.pad(x64[:, None], (n // 2, n // 2), mode="reflect")[:, 0]
        fr = xp.unfold(-1, n, hop)[:, :nf] * win.double()
        fr.backward(dfr.double())
        return dict(frames=fr.detach(), dx=x64.grad, dx_acc=base.double() + x64.grad)
    want = _ref("stft_frames", ref)
    xd, dd, wd = P.i(x), P.i(dfr), P.i(win)
    fr, dx, acc = P.o(rows, nf, n), P.o(rows, t), P.io(base)
    L.check(L.lib.rh_stft_frame_fwd_f32(L.ptr(xd), L.ptr(wd), rows, t, n, hop, nf, L.ptr(fr), _s()), "stft_frame_fwd")
    L.check(L.lib.rh_stft_frame_bwd_f32(L.ptr(dd), L.ptr(wd), rows, t, n, hop, nf, L.ptr(dx), _s()), "stft_frame_bwd")
    L.check(L.lib.rh_stft_frame_bwd_acc_f32(L.ptr(dd), L.ptr(wd), rows, t, n, hop, nf, L.ptr(acc), 1, _s()), "stft_frame_bwd_acc")
    return dict(frames=fr, dx=dx, dx_acc=acc), want


def row_feature_matching(P, half, relative):
    """rh_feature_matching_fwd_f32 / _bwd_f32 over three feature maps of 2 x ``half`` elements (real half first); half = 64 takes
    the 16-byte path of feature_match.hip at aligned pointers, half = 67 never."""
    import rave_oracle as O
    L = _lib()
    g = _gen(1000 + half)
    fs = [torch.randn(2, half, generator=g) for _ in range(3)]
    wts = [0.5, 0.3, 0.2]

    def ref():
        f64 = [f.double().requires_grad_(True) for f in fs]
        loss = sum(w * O.mean_difference(f[0], f[1], "L1", relative) for w, f in zip(wts, f64))
        loss.backward(torch.tensor(1.3, dtype=torch.float64))
        out = dict(loss=loss.detach().reshape(1))
        out.update({f"df{i}": f.grad for i, f in enumerate(f64)})
        return out
    want = _ref(("fm", half, relative), ref)
    fd = [P.i(f) for f in fs]
    dfs = [P.o(2, half) for _ in fs]
    gd = P.i(torch.tensor([1.3]))
    arr = (L.FmItem * 3)()
    for i in range(3):
        arr[i].f, arr[i].df, arr[i].half = fd[i].data_ptr(), dfs[i].data_ptr(), half
        arr[i].w = wts[i] if relative else wts[i] / half
    nb = L.lib.rh_feature_matching_workspace_bytes(arr, 3)
    ws = torch.empty(max(nb // 4, 4), device=P.dev)
    sums, out = P.o(3, 2), P.o(1)
    L.check(L.lib.rh_feature_matching_fwd_f32(arr, 3, int(relative), L.ptr(ws), nb, L.ptr(sums), L.ptr(out), _s()), "fm_fwd")
    L.check(L.lib.rh_feature_matching_bwd_f32(arr, 3, int(relative), L.ptr(sums), L.ptr(gd), _s()), "fm_bwd")
    got = dict(loss=out)
    got.update({f"df{i}": d for i, d in enumerate(dfs)})
    return got, want



def row_pqmf_fold(P, causal):
    """The four PQMF transforms in their folded form (rh_pqmf_fold_k1_f32 / _k2_f32: no alignment check, wide stores justified by
    the row length), rows = 2, T = 1024 + 16, with the offsets rave_amd.ops derives for each transform."""
    import rave_oracle as O
    from rave_amd import pqmf
    L = _lib()
    sd = O.pqmf_buffers(100, 16)
    wf, wi = sd["forward_conv.weight"], sd["inverse_conv.weight"]
    tab, lpad = pqmf.fold_tables(sd["h"], sd["hk"])
    mode = "causal" if causal else "centered"
    T, K, K2 = 1040, wf.shape[-1], wi.shape[-1]
    pf, pi = O.get_padding(K, mode=mode), O.get_padding(K2, mode=mode)
    nfr = (T + pf[0] + pf[1] - K) // 16 + 1
    n_out = nfr + pi[0] + pi[1] - K2 + 1
    g = _gen(960 + int(causal))
    x = O.synthetic_batch(2, 1, T, seed=7)
    cy, yin, cx = torch.randn(2, 16, nfr, generator=g), torch.randn(2, 16, nfr, generator=g), torch.randn(2, 1, n_out * 16, generator=g)

    def ref():
        x64, y64 = x.double().requires_grad_(True), yin.double().requires_grad_(True)
        ya = O.pqmf_analysis(x64, wf.double(), causal)
        ya.backward(cy.double())
        xs = O.pqmf_synthesis(y64, wi.double(), causal)
        xs.backward(cx.double())
        return dict(y=ya.detach(), dx=x64.grad, xs=xs.detach(), dy=y64.grad)
    want = _ref(("pqmf_fold", causal), ref)
    xd, cyd, yd, cxd, td = P.i(x), P.i(cy), P.i(yin), P.i(cx), P.i(tab.float())
    y, dx, xs, dy = P.o(2, 16, nfr), P.o(2, 1, T), P.o(2, 1, n_out * 16), P.o(2, 16, nfr)
    s = _s()
    L.check(L.lib.rh_pqmf_fold_k1_f32(L.ptr(xd), L.ptr(td), 2, T, nfr, lpad - pf[0], 1.0, L.ptr(y), s), "fold_k1 analysis")
    L.check(L.lib.rh_pqmf_fold_k2_f32(L.ptr(cyd), L.ptr(td), 2, nfr, T, pf[0] - lpad, 1.0, L.ptr(dx), s), "fold_k2 analysis bwd")
    L.check(L.lib.rh_pqmf_fold_k2_f32(L.ptr(yd), L.ptr(td), 2, nfr, n_out * 16, 496 - 16 * pi[0] - lpad, 16.0, L.ptr(xs), s), "fold_k2 synthesis")
    L.check(L.lib.rh_pqmf_fold_k1_f32(L.ptr(cxd), L.ptr(td), 2, n_out * 16, nfr, lpad - (496 - 16 * pi[0]), 16.0, L.ptr(dy), s),
            "fold_k1 synthesis bwd")
    return dict(y=y, dx=dx, xs=xs, dy=dy), want


def _loss_signals(rows=3, t=1000):
    """y = 0.6 x + small noise keeps |Sy| < |Sx| at (almost) every bin, so that no sign term of the log distance flips under
    rounding (tests/test_gpu_stft_loss.py: test_stft_loss_value_and_smooth_gradient_vs_f64)."""
    g = _gen(rows * 13 + t)
    x = torch.randn(rows, t, generator=g)
    return x, 0.6 * x + 0.01 * torch.randn(rows, t, generator=g)


def _norm_window(n):
    w = torch.hann_window(n, dtype=torch.float64)
    return w / w.pow(2).sum().sqrt()


def _distance64(sx, sy, eps):
    return ((sx - sy) ** 2).mean() / (sx ** 2).mean() + (torch.log(sx + eps) - torch.log(sy + eps)).abs().mean()


def row_stft_loss(P, n_fft):
    """rh_stft_loss_fwd_f32 / _bwd_f32 on one scale, rows = 3, t = 1000, eps = 1e-2, against torch.stft in f64 under the bounds of
    test_stft_loss_value_and_smooth_gradient_vs_f64 (value 2e-6, gradients 5e-5)."""
    L = _lib()
    rows, t, eps = 3, 1000, 1e-2
    x, y = _loss_signals(rows, t)
    w64 = _norm_window(n_fft)

    def ref():
        x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
        sx = torch.stft(x64, n_fft, n_fft // 4, n_fft, w64, center=True, pad_mode="reflect", return_complex=True).abs()
        sy = torch.stft(y64, n_fft, n_fft // 4, n_fft, w64, center=True, pad_mode="reflect", return_complex=True).abs()
        d = _distance64(sx, sy, eps)
        d.backward(torch.tensor(0.8, dtype=torch.float64))
        return dict(value=d.detach().reshape(1), dx=x64.grad, dy=y64.grad)
    want = _ref(("stft_loss", n_fft), ref)
    assert L.lib.rh_stft_loss_supported(n_fft, n_fft // 4, t, rows) == 1
    a = torch.arange(n_fft, dtype=torch.float64) * (-2.0 * math.pi / n_fft)
    tw = torch.stack([torch.cos(a), torch.sin(a)], -1).float()
    xd, yd, wd, twd, gd = P.i(x), P.i(y), P.i(w64.float()), P.i(tw), P.i(torch.tensor([0.8]))
    sums, dx, dy = P.o(3), P.o(rows, t), P.o(rows, t)
    nb = int(L.lib.rh_stft_loss_workspace_bytes(n_fft, t, rows))
    ws = torch.empty(max(nb, 16) // 4, device=P.dev)
    s = _s()
    L.check(L.lib.rh_stft_loss_fwd_f32(L.ptr(xd), L.ptr(yd), L.ptr(wd), L.ptr(twd), rows, t, n_fft, eps, L.ptr(sums), L.ptr(ws), nb, s),
            "stft_loss_fwd")
    L.check(L.lib.rh_stft_loss_bwd_f32(L.ptr(xd), L.ptr(yd), L.ptr(wd), L.ptr(twd), rows, t, n_fft, eps, L.ptr(sums), L.ptr(gd), L.ptr(dx),
                                       L.ptr(dy), 0, s), "stft_loss_bwd")
    torch.cuda.synchronize()
    n_complex = rows * (t // (n_fft // 4) + 1) * (n_fft // 2 + 1)
    sm = sums.double().cpu()
    assert torch.isfinite(sums).all()
    return dict(value=(sm[0] / sm[1] + sm[2] / n_complex).reshape(1), dx=dx, dy=dy), want


def row_spectral_distance(P):
    """rh_spectral_distance_fwd_f32 / _bwd_f32 on the complex spectra (n_fft = 128) of the same signals, eps = 1e-2: value within
    2e-5, gradients within 2e-4 (the bounds of test_fused_spectral_distance_vs_torch)."""
    L = _lib()
    eps, n_fft = 1e-2, 128
    x, y = _loss_signals()
    w = _norm_window(n_fft).float()
    rx = torch.view_as_real(torch.stft(x, n_fft, 32, n_fft, w, center=True, pad_mode="reflect", return_complex=True)).contiguous()
    ry = torch.view_as_real(torch.stft(y, n_fft, 32, n_fft, w, center=True, pad_mode="reflect", return_complex=True)).contiguous()
    n = rx.numel() // 2

    def ref():
        a, b = rx.double().requires_grad_(True), ry.double().requires_grad_(True)
        d = _distance64(torch.view_as_complex(a).abs(), torch.view_as_complex(b).abs(), eps)
        d.backward(torch.tensor(0.8, dtype=torch.float64))
        return dict(value=d.detach().reshape(1), dsx=a.grad, dsy=b.grad)
    want = _ref("spectral_distance", ref)
    xd, yd, gd = P.i(rx), P.i(ry), P.i(torch.tensor([0.8]))
    sums, dsx, dsy = P.o(3), P.o(*rx.shape), P.o(*ry.shape)
    nb = int(L.lib.rh_spectral_distance_workspace_bytes())
    ws = torch.empty(max(nb, 16) // 4, device=P.dev)
    L.check(L.lib.rh_spectral_distance_fwd_f32(L.ptr(xd), L.ptr(yd), n, eps, L.ptr(sums), L.ptr(ws), nb, _s()), "spectral_distance_fwd")
    L.check(L.lib.rh_spectral_distance_bwd_f32(L.ptr(xd), L.ptr(yd), L.ptr(sums), L.ptr(gd), n, eps, L.ptr(dsx), L.ptr(dsy), 0, _s()),
            "spectral_distance_bwd")
    torch.cuda.synchronize()
    sm = sums.double().cpu()
    assert torch.isfinite(sums).all()
    return dict(value=(sm[0] / sm[1] + sm[2] / n).reshape(1), dsx=dsx, dsy=dsy), want


VQ = dict(n=256, k=64, d=16)


def _vq_data(k=None):
    k = k or VQ["k"]
    g = _gen(1100 + k)
    x = 0.3 * torch.randn(VQ["n"], VQ["d"], generator=g)
    embed = 0.3 * torch.randn(k, VQ["d"], generator=g)
    return x, embed, g


def row_vq_ema_update(P):
    """rh_vq_ema_update_f32 at 256 vectors x 64 codes x 16 dims (cluster_size and embed_avg updated in place, embed written):
    measured row."""
    L = _lib()
    x, embed, g = _vq_data()
    ind = torch.cdist(x.double(), embed.double()).argmin(1)
    cs0, avg0 = torch.rand(VQ["k"], generator=g) * 4 + 0.5, 0.3 * torch.randn(VQ["k"], VQ["d"], generator=g)
    decay, epsilon = 0.8, 1e-5

    def ref():
        onehot = F.one_hot(ind, VQ["k"]).double()
        cs = cs0.double() * decay + onehot.sum(0) * (1 - decay)
        avg = avg0.double() * decay + (x.double().t() @ onehot).t() * (1 - decay)
        smoothed = (cs + epsilon) / (cs.sum() + VQ["k"] * epsilon) * cs.sum()
        return dict(cluster_size=cs, embed_avg=avg, embed=avg / smoothed.unsqueeze(1))
    want = _ref("vq_ema", ref)
    xd, idd = P.i(x), P.i(ind)
    cs, avg, em = P.io(cs0), P.io(avg0), P.o(VQ["k"], VQ["d"])
    L.check(L.lib.rh_vq_ema_update_f32(L.ptr(xd), L.ptr(idd), VQ["n"], VQ["d"], VQ["k"], decay, epsilon, L.ptr(cs), L.ptr(avg), L.ptr(em),
                                       _s()), "vq_ema_update")
    return dict(cluster_size=cs, embed_avg=avg, embed=em), want



ROWS = {
    # name: (row function, arguments, bound: a tolerance, or None = "measured": 2 x the aligned arrangement's own error)
    "weight_norm_cols12": (row_weight_norm, (12,), TOL_OP),
    "weight_norm_cols13": (row_weight_norm, (13,), TOL_OP),
    "weight_norm_bwd_batched": (row_weight_norm_batched, (), TOL_OP),
    "reduce_partials_n65536_Z4": (row_reduce_partials, (65536, 4), TOL_OP),
    "reduce_partials_n1001_Z3": (row_reduce_partials, (1001, 3), TOL_OP),
    "amp_tanh_L100": (row_amp_tanh, (100,), TOL_OP),
    "amp_tanh_L101": (row_amp_tanh, (101,), TOL_OP),
    "snake_L100": (row_snake, (100,), None),
    "snake_L101": (row_snake, (101,), None),
    "act_bwd_and_bias_L100": (row_act_bwd, (100,), TOL_OP),
    "act_bwd_and_bias_L101": (row_act_bwd, (101,), TOL_OP),
    "avgpool2_L100": (row_avgpool2, (100,), TOL_OP),
    "avgpool2_L101": (row_avgpool2, (101,), TOL_OP),
}
for _name in CONVS:
    ROWS[f"conv1d_{_name}_x6"] = (row_conv1d, (_name, True), TOL_OP)
    ROWS[f"conv1d_{_name}_f32"] = (row_conv1d, (_name, False), TOL_OP)
for _name in CONV2DS:
    ROWS[f"conv2d_{_name}_x6"] = (row_conv2d, (_name, 1), TOL_OP)
    ROWS[f"conv2d_{_name}_f32"] = (row_conv2d, (_name, 0), TOL_OP)
ROWS.update({
    "residual_unit_C32_L64": (row_residual_unit, (), TOL_OP),
    "pqmf_direct_centered": (row_pqmf, (False,), TOL_OP),
    "pqmf_direct_causal": (row_pqmf, (True,), TOL_OP),
    "adain_L100": (row_adain, (100,), None),
    "adain_L101": (row_adain, (101,), None),
    "reparam_L100": (row_reparam, (100,), TOL_OP),
    "reparam_L101": (row_reparam, (101,), TOL_OP),
    "stft_frames_t1000_n128": (row_stft_frames, (), 1e-5),          # the bound of test_stft_framing_matches_torch_stft
    "feature_matching_half64": (row_feature_matching, (64, False), TOL_OP),
    "feature_matching_half64_relative": (row_feature_matching, (64, True), TOL_OP),
    "feature_matching_half67": (row_feature_matching, (67, False), TOL_OP),
    "feature_matching_half67_relative": (row_feature_matching, (67, True), TOL_OP),
    "pqmf_fold_centered": (row_pqmf_fold, (False,), TOL_OP),
    "pqmf_fold_causal": (row_pqmf_fold, (True,), TOL_OP),
    "stft_loss_n128": (row_stft_loss, (128,), dict(value=2e-6, dx=5e-5, dy=5e-5)),
    "stft_loss_n512": (row_stft_loss, (512,), dict(value=2e-6, dx=5e-5, dy=5e-5)),
    "spectral_distance_n128": (row_spectral_distance, (), dict(value=2e-5, dsx=2e-4, dsy=2e-4)),
    "vq_ema_update": (row_vq_ema_update, (), None),
})


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(ROWS))
def test_entry_point_at_misaligned_operands_vs_f64(dev, row):
    fn, args, bound = ROWS[row]
    aligned_err, aligned_out = {}, {}
    for which, off in ARRANGEMENTS:
        P = Place(dev, which, off)
        got, want = fn(P, *args)
        torch.cuda.synchronize()
        assert (which == "aligned") == (not P.carved)
        for v in P.carved:
            assert v.data_ptr() % 16 == (4 * off if v.element_size() <= 4 else 8)
            assert guards_intact(v), (row, which, off, tuple(v.shape))
        for k, t in got.items():
            assert torch.isfinite(t).all(), (row, which, off, k)
            e = rel_l2(t, want[k])
            own = bound.get(k) if isinstance(bound, dict) else bound
            if which == "aligned":
                aligned_err[k], aligned_out[k] = e, t.clone()
                lim = TOL_OP if own is None else own
            else:
                lim = 2.0 * aligned_err[k] if own is None else own
            same = "same bits as aligned" if torch.equal(t, aligned_out[k]) else f"differs from aligned by {rel_l2(t, aligned_out[k]):.2e}"
            print(f"{row} {which}+{off} {k}: rel-L2 against f64 {e:.3e} (bound {lim:.3e}); {same}")
            assert e <= lim, (row, which, off, k, e, lim)


ADAM_SIZES = (1, 5, 2047, 2049)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_adam_step_with_parameter_and_both_moments_misaligned(dev, off):
    """rh_adam_step_f32 with p, m AND v off a 16-byte boundary (the existing test offsets the gradient only; adam.hip takes its
    16-byte path from the four pointers together), gradients aligned and misaligned in turn: three steps against
    torch.optim.Adam under the bounds of test_fused_adam_kernel_matches_torch_adam."""
    from rave_amd.optim import FusedAdam
    gen = _gen(11)
    base = [torch.randn(n, generator=gen) for n in ADAM_SIZES]
    carved = []

    def put(t):
        v = carve(t.to(dev), off)
        carved.append(v)
        return v

    pa = [torch.nn.Parameter(put(b)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    lr_a = torch.tensor(1e-3, device=dev)
    oa, ob = FusedAdam(pa, lr_a, (.5, .9)), torch.optim.Adam(pb, 1e-3, (.5, .9))
    for p in pa:
        assert p.data_ptr() % 16 == 4 * off
        oa.state[p]["step"] = torch.zeros((), device=dev)
        oa.state[p]["exp_avg"], oa.state[p]["exp_avg_sq"] = put(torch.zeros_like(p.data)), put(torch.zeros_like(p.data))
        assert oa.state[p]["exp_avg"].data_ptr() % 16 == 4 * off and oa.state[p]["exp_avg_sq"].data_ptr() % 16 == 4 * off
    for it in range(3):
        for a, b in zip(pa, pb):
            g = torch.randn(a.shape, generator=gen) * (10.0 ** (it - 1))
            a.grad = put(g) if it % 2 == 0 else g.to(dev)
            b.grad = g.to(dev)
        oa.step(); ob.step()
        torch.cuda.synchronize()
        for a, b in zip(pa, pb):
            assert a.data_ptr() % 16 == 4 * off
            assert rel_l2(a.detach(), b.detach()) < 2e-7, (a.numel(), it)
    for a, b in zip(pa, pb):
        assert rel_l2(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) < 1e-6
        assert rel_l2(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) < 1e-6
        assert float(oa.state[a]["step"]) == 3.0
    for v in carved:
        assert guards_intact(v), tuple(v.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wp3", "wp1"])
def test_residual_unit_refuses_misaligned_packed_weights_and_writes_nothing(dev, which):
    """The one alignment requirement of the ABI (include/rave_hip.h, at rh_residual_unit_fwd_f32): the packed weights of the
    fused unit are read with 16-byte buffer loads and must be 16-byte aligned.  A packed operand one float off the boundary
    is answered with RH_ERR_INVALID before anything is enqueued: h and y keep every bit."""
    L = _lib()
    x, w3, w1, d3, d1, (wp3, wp1) = _unit_setup(dev)
    if which == "wp3":
        wp3 = carve(wp3, 1)
    else:
        wp1 = carve(wp1, 1)
    xd = x.to(dev)
    h, y = carve(torch.full((2, 32, 64), float("nan")).to(dev), 0), carve(torch.full((2, 32, 64), float("nan")).to(dev), 0)
    sl = torch.zeros(L.lib.rh_x6_range_words(), dtype=torch.int32, device=dev)
    L.check(L.lib.rh_amax_f32(L.ptr(xd), xd.numel(), L.ptr(sl), _s()), "amax")
    L.lib.rh_x6_set_ranges(None, L.ptr(sl), None, None)
    rc = L.lib.rh_residual_unit_fwd_f32(C.byref(d3), C.byref(d1), L.ptr(xd), L.ptr(wp3), L.ptr(wp1), L.ptr(h), L.ptr(y), _s())
    torch.cuda.synchronize()
    assert rc == -1, rc                                   # RH_ERR_INVALID
    assert b"misaligned" in L.lib.rh_last_error()
    assert torch.isnan(h).all() and torch.isnan(y).all() and guards_intact(h) and guards_intact(y)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["x", "embed"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("k", [64, 256])
def test_vq_assign_with_a_misaligned_operand_gives_the_bits_of_the_matrix_core_path(dev, k, which, off):
    """rh_vq_assign_ws_f32 at 256 vectors x 16 dims: with ``x`` or ``embed`` off a 16-byte boundary the host (vq.hip, the
    workspace branch) falls back to the one-launch kernel, for which the header promises the same distances: indices,
    residual, running sum and loss partials must be torch.equal to the aligned run; the outputs are carved as well, and every
    guard holds.  64 codes: the library takes the one-launch kernel at every pointer (the matrix-core search needs a
    multiple of 256 codes: rh_vq_assign_workspace_bytes is 0).  256 codes, the smallest codebook at which the branch exists:
    the aligned run is the two-launch matrix-core path (asserted), the misaligned ones the fallback."""
    L = _lib()
    x, embed, _ = _vq_data(k)
    n, d = VQ["n"], VQ["d"]
    nbytes = L.lib.rh_vq_assign_workspace_bytes(n, d, k)
    assert (nbytes > 0) == (k == 256)                             # at 256 codes the aligned run really is the matrix-core path
    qs0 = torch.full((n, d), 0.25)

    def run(xd, ed, carve_out):
        put = (lambda t: carve(t.to(dev), off if t.element_size() <= 4 else 2)) if carve_out else (lambda t: t.to(dev))
        ind, res, qsum = put(torch.full((n,), -1, dtype=torch.int64)), put(torch.full((n, d), float("nan"))), put(qs0)
        parts = put(torch.full((L.lib.rh_vq_loss_partials(n),), float("nan")))
        ws = torch.empty(max(nbytes, 16) // 4, device=dev)
        L.check(L.lib.rh_vq_assign_ws_f32(L.ptr(xd), L.ptr(ed), n, d, k, L.ptr(ind), L.ptr(res), L.ptr(qsum), L.ptr(parts), L.ptr(ws),
                                          nbytes, _s()), "vq_assign_ws")
        torch.cuda.synchronize()
        return ind, res, qsum, parts

    base = run(x.to(dev), embed.to(dev), False)
    ref = torch.cdist(x.double(), embed.double())
    top = ref.topk(2, dim=1, largest=False).values
    clear = (top[:, 1] - top[:, 0]) > 1e-5 * top[:, 1]
    assert int(clear.sum()) > 0.98 * n and torch.equal(base[0].cpu()[clear], ref.argmin(1)[clear])
    xc = carve(x.to(dev), off) if which == "x" else x.to(dev)
    ec = carve(embed.to(dev), off) if which == "embed" else embed.to(dev)
    assert (xc if which == "x" else ec).data_ptr() % 16 == 4 * off
    for carve_out in (False, True):
        got = run(xc, ec, carve_out)
        for name, a, b in zip(("indices", "residual", "quantized_sum", "loss_partials"), got, base):
            assert torch.equal(a, b), (name, which, off, carve_out)
        assert guards_intact(xc if which == "x" else ec)
        if carve_out:
            for t in got:
                assert t.data_ptr() % 16 == (4 * off if t.element_size() <= 4 else 8) and guards_intact(t)


class _RedirectOut:
    """Runs rave_amd.data.GpuBatchFeed.sample with the C call's ``out`` argument pointed at a tensor of the test's choosing
    (sample() allocates its own, aligned one): the argument at ``index`` of ``name`` is replaced on the way into the library."""

    def __init__(self, name, index, tensor):
        self.name, self.index, self.tensor = name, index, tensor

    def __enter__(self):
        L = _lib()
        self.real = getattr(L.lib, self.name)

        def call(*args):
            args = list(args)
            args[self.index] = self.tensor.data_ptr()
            return self.real(*args)
        L.lib.__dict__[self.name] = call
        return self

    def __exit__(self, *a):
        _lib().lib.__dict__[self.name] = self.real


FEED_LENGTH, FEED_N = 5000, 2048
FEED_ANGLES = [0.05, None, 0.2]
FEED_RATIOS = [(13, 10), None, (4, 6)]


def _feed_reference(pcm, noise, items, in_points, ratios, dtype):
    """The reference's per-item chain for the injected draws (tests/test_gpu_feed_pitch.py: chain), one channel; float64 before
    the last cast."""
    import numpy as np
    from scipy.signal import lfilter, resample_poly
    out = np.empty((len(items), FEED_N), dtype=np.float64)
    for b in range(len(items)):
        x = (pcm[items[b], 0].astype(np.float32) / (2 ** 15 - 1)).astype(dtype)
        if ratios[b] is not None:
            x = resample_poly(x, ratios[b][0], ratios[b][1], padtype="mean", axis=-1)
        x = x[in_points[b]:in_points[b] + FEED_N]
        if FEED_ANGLES[b] is not None:
            z0 = .99 * np.exp(1j * FEED_ANGLES[b])
            aa = [1.0, -2.0 * float(np.real(z0)), float(abs(z0) ** 2)]
            bb = [float(abs(z0) ** 2), -2.0 * float(np.real(z0)), 1.0]
            x = lfilter(bb, aa, x)
        out[b] = x.astype(np.float64) + noise[b].astype(np.float64) / 2 ** 16
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pitched", [False, True], ids=["rh_feed_batch_i16_f32", "rh_feed_batch_resample_i16_f32"])
def test_batch_feed_with_noise_and_out_misaligned(dev, pitched):
    """3 rows x 2048 samples of the data feed with ``noise`` and / or ``out`` 1, 2, 3 floats off a 16-byte boundary, against the
    reference's chain restated with scipy (float64): the bound of test_gpu_batch_feed_matches_the_reference_transform_chain
    (2e-6 max(1, max |ref|)), for the pitched feed plus the reference's own float32 deviation as in
    test_pitched_feed_matches_the_reference_chain; and the same bits as the aligned run."""
    import numpy as np
    from rave_amd import data as D
    rng = np.random.default_rng(3)
    pcm = (rng.integers(-12000, 12000, size=(4, 1, FEED_LENGTH)) + 3000).astype(np.int16)
    noise = rng.random((3, FEED_N)).astype(np.float32)
    items = np.array([2, 0, 3])
    ratios = FEED_RATIOS if pitched else [None, None, None]
    n_res = [FEED_LENGTH if r is None else -(-FEED_LENGTH * r[0] // r[1]) for r in ratios]
    in_points = np.array([0, 777, n_res[2] - FEED_N])
    feed = D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=44100, seed=1, **(dict(rand_pitch=(0.6, 1.4)) if pitched else {}))
    draws = (items, in_points, FEED_ANGLES, ratios) if pitched else (items, in_points, FEED_ANGLES)
    name, index = ("rh_feed_batch_resample_i16_f32", 21) if pitched else ("rh_feed_batch_i16_f32", 7)
    ref64 = _feed_reference(pcm, noise, items, in_points, ratios, np.float64)
    own = np.abs(_feed_reference(pcm, noise, items, in_points, ratios, np.float32).astype(np.float32) - ref64).max(1) if pitched \
        else np.zeros(3)
    base = feed.sample(3, FEED_N, draws=draws, noise=torch.from_numpy(noise)).reshape(3, FEED_N)
    torch.cuda.synchronize()

    def check(got, tag):
        assert torch.isfinite(got).all(), tag
        g = got.double().cpu().numpy()
        for b in range(3):
            err, bound = np.abs(g[b] - ref64[b]).max(), own[b] + 2e-6 * max(1.0, np.abs(ref64[b]).max())
            print(f"{name} {tag} row {b}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (tag, b)
    check(base, "aligned")
    for off in (1, 2, 3):
        for cn, co in ((True, False), (False, True), (True, True)):
            nz = carve(torch.from_numpy(noise).to(dev), off) if cn else torch.from_numpy(noise).to(dev)
            out = carve(torch.full((3, FEED_N), float("nan")).to(dev), off) if co else None
            if co:
                with _RedirectOut(name, index, out):
                    feed.sample(3, FEED_N, draws=draws, noise=nz)
            else:
                out = feed.sample(3, FEED_N, draws=draws, noise=nz).reshape(3, FEED_N)
            torch.cuda.synchronize()
            tag = f"noise{'+' + str(off) if cn else ''} out{'+' + str(off) if co else ''}"
            check(out, tag)
            assert torch.equal(out, base), tag
            for t, c in ((nz, cn), (out, co)):
                if c:
                    assert t.data_ptr() % 16 == 4 * off and guards_intact(t), tag
