"""Range slots of the f16-piece ("x6") kernels (csrc/common.hpp, include/rave_hip.h: rh_x6_set_ranges), checked directly.

A slot that is too SMALL overflows the f16 pieces (Inf / NaN with return code 0); one that is much too LARGE flushes the tensor
into the f16 subnormals (quietly less accurate).  End-to-end parity tests see neither below a factor of 2, so this file checks:

A. every producer publishes EXACTLY max |output| (each takes the maximum of the values it stores), with the maximum placed where
   a producer is most likely to miss it (bias / residual term, negative sign, last ragged column of the last batch item, beyond
   the first workgroups, odd offsets), and the kernel family each case exercises asserted;
B. the consumer at the edges of the scale scheme against fp64 (quiet clips, zero / impulse / huge / tiny / subnormal / non-finite
   tensors);
C. the slot lifetime rules of rave_amd/_ranges.py (pools around a recorded step, version counters and views, slots computed on the
   weight-gradient side stream, pool exhaustion in the middle of a step);
D. the thread-local state rh_x6_set_ranges / rh_defer_reduce / rh_set_kernel_events arm is consumed by a call that fails.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import rave_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def f16(ops):
    if ops.L.lib.rh_x6_uses_ranges() != 1:
        pytest.skip("comparison build (three bf16 pieces): no scales, no range slots")
    return ops


def _zslot(ops, dev):
    return torch.zeros(ops._RANGE_WORDS, device=dev, dtype=torch.int32)


def _smax(slot) -> float:
    """max |x| a slot records (one word per 128-byte line, common.hpp: kRangeWords x kRangeStride)."""
    return float(slot.view(torch.float32).max())


def _amax_slot(ops, t):
    s = _zslot(ops, t.device)
    ops.L.check(ops.L.lib.rh_amax_f32(ops.L.ptr(t), t.numel(), ops.L.ptr(s), ops.L.stream()), "amax")
    return s


def _assert_publishes(slot, y, what):
    """The contract (slot >= max |y|, hard) and what every publisher does (slot == max |y| bit for bit)."""
    torch.cuda.synchronize()
    m = float(y.detach().abs().max())
    got = _smax(slot)
    assert got >= m, (what, got, m)
    assert got == m, (what, got, m)


def _plan(ops, d, which, has_bias, has_add):
    out = (C.c_int32 * 8)()
    ops.L.check(ops.L.lib.rh_conv1d_plan_info(C.byref(d), which, int(has_bias), int(has_add), out), "plan_info")
    return tuple(out)


def _seed(name: str) -> int:
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def _ws(ops, nbytes, dev):
    return torch.empty(max(nbytes, 4) // 4, device=dev, dtype=torch.float32)


# --------------------------------------------------------------------------------------------------------------- A. conv1d
# (name, B, Cin, Cout, L, k, stride, dil, pad, act, bias, residual, transposed, arm input slot, workspace, family, K slices)
#   family: what rh_conv1d_plan_info reports for the geometry (1 = f16 pieces, 2 = small-C vector kernels, 0 = f32 MFMA);
#   "arm input slot" False on a family-1 geometry = the f32-input MFMA kernels of the igemm-DMA path (no input slot)
#   K slices: ">1" = a split launch (partials combined by the K-split reduction), 1 = unsplit, None = not an x6 plan
PRODUCER_CASES = [
    ("smallc stem Cin=1 bias", 4, 1, 96, 1000, 15, 4, 1, (7, 7), 0, True, False, False, False, True, 2, None),
    ("smallc stereo", 2, 2, 64, 2050, 15, 4, 1, (7, 7), 0, False, False, False, False, True, 2, None),
    ("f32 igemm odd sizes", 1, 130, 70, 33, 5, 1, 2, (4, 4), 0, False, False, False, False, True, 0, None),
    ("f32 igemm ragged bias+residual", 2, 6, 12, 70, 3, 1, 3, (3, 3), 1, True, True, False, False, True, 0, None),
    ("igemm-DMA f32 (no input slot)", 2, 96, 96, 257, 3, 1, 9, (9, 9), 1, False, True, False, False, True, 1, ">1"),
    ("igemm-DMA f32 split-K", 9, 384, 768, 32, 3, 1, 1, (1, 1), 1, False, False, False, False, True, 1, ">1"),
    ("igemm-DMA f32 long unsplit", 32, 96, 96, 40003, 3, 1, 1, (1, 1), 0, False, False, False, False, True, 1, 1),
    ("x6 dilated k3", 2, 96, 96, 257, 3, 1, 9, (9, 9), 1, False, False, False, True, True, 1, ">1"),
    ("x6 bias+residual causal", 3, 192, 96, 64, 3, 1, 3, (6, 0), 1, True, True, False, True, True, 1, ">1"),
    ("x6 split-K", 9, 384, 768, 32, 3, 1, 1, (1, 1), 1, False, False, False, True, True, 1, ">1"),
    ("x6 split-K without workspace", 9, 384, 768, 32, 3, 1, 1, (1, 1), 1, False, True, False, True, False, 1, ">1"),
    ("x6 > 4096 workgroups", 32, 96, 96, 40003, 3, 1, 1, (1, 1), 0, False, False, False, True, True, 1, 1),
    ("transposed x4", 2, 64, 32, 129, 8, 4, 1, (2, 2), 1, True, False, True, True, True, 1, None),
]


def _producer_operands(case, dev, gen):
    name, B, Ci, Co, L, k, s, dil, pad, act, has_b, has_r, tr, arm, use_ws, fam, ks = case
    from rave_amd.ops import ConvGeom
    g = ConvGeom(stride=s, dilation=dil, pad_left=pad[0], pad_right=pad[1], act=act, slope=0.2, transposed=tr)
    l_out = g.out_len(L, k)
    x = torch.randn(B, Ci, L, generator=gen) * 0.01
    w = (torch.randn(Ci, Co, k, generator=gen) if tr else torch.randn(Co, Ci, k, generator=gen)) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=gen) * 0.01 if has_b else None
    r = torch.randn(B, Co, l_out, generator=gen) * 0.01 if has_r else None
    # the true maximum |y| where a publisher is most likely to miss it: a negative residual / bias term far above the conv
    # part, in the last column of the last batch item; without either, a spike of the LAST input channel at the last position:
    # only the last K slice of a split launch sees it
    if has_r:
        r[-1, -1, -1] = -1000.0
    elif has_b:
        b[-1] = -300.0
    else:
        x[-1, -1, -1] = -50.0
    return g, l_out, x.to(dev), w.to(dev), None if b is None else b.to(dev), None if r is None else r.to(dev)


@pytest.mark.parametrize("case", PRODUCER_CASES, ids=[c[0] for c in PRODUCER_CASES])
def test_conv1d_forward_publishes_exactly_max_abs_y(f16, dev, case):
    ops = f16
    L = ops.L
    name, B, Ci, Co, Lx, k, s, dil, pad, act, has_b, has_r, tr, arm, use_ws, fam, ks = case
    g, l_out, x, w, b, r = _producer_operands(case, dev, torch.Generator().manual_seed(_seed(name)))
    d = ops._desc(g, B, Ci, Co, Lx, l_out, k)
    info = _plan(ops, d, 0, has_b, has_r)
    if fam is not None:
        assert info[0] == fam, (name, info)
    if ks == ">1":
        assert info[4] > 1, (name, info)
    elif ks == 1:
        assert info[4] == 1, (name, info)
    if "4096" in name:
        assert info[7] > 4096, (name, info)
    st = L.stream()
    wp_f, _, _ = ops._pack(d, w, None, False, dev, st)
    rin = _amax_slot(ops, x) if arm else None
    rout = _zslot(ops, dev)
    y = torch.empty(B, Co, l_out, device=dev)
    nb = L.lib.rh_conv1d_fwd_workspace_bytes(C.byref(d)) if use_ws else 0
    ws = _ws(ops, nb, dev) if nb > 0 else None
    L.lib.rh_x6_set_ranges(None, L.ptr(rin), L.ptr(rout), None)
    L.check(L.lib.rh_conv1d_fwd_f32(C.byref(d), L.ptr(x), L.ptr(wp_f), L.ptr(b), None, L.ptr(r), L.ptr(y), L.ptr(ws), nb, st),
            name)
    assert torch.isfinite(y).all(), name
    _assert_publishes(rout, y, name)


DGRAD_CASES = [c for c in PRODUCER_CASES if not c[0].startswith(("smallc stereo", "f32 igemm ragged"))]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv1d_data_gradient_publishes_exactly_max_abs_dx(f16, dev, case):
    ops = f16
    L = ops.L
    name, B, Ci, Co, Lx, k, s, dil, pad, act, has_b, has_r, tr, arm, use_ws, fam, ks = case
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    g, l_out, x, w, _, _ = _producer_operands(case, dev, gen)
    d = ops._desc(g, B, Ci, Co, Lx, l_out, k)
    dy = (torch.randn(B, Co, l_out, generator=gen) * 0.01)
    add = torch.randn(B, Ci, Lx, generator=gen) * 0.01 if has_r else None
    if add is not None:
        add[-1, -1, -1] = -1000.0         # the maximum in the added term, negative, last column of the last item
    else:
        dy[-1, -1, -1] = -50.0
    dy = dy.to(dev)
    add = None if add is None else add.to(dev)
    fam1 = L.lib.rh_conv1d_kernel_family(C.byref(d), 1, 0, int(add is not None))
    info = _plan(ops, d, 1, False, add is not None)
    assert info[0] == fam1
    st = L.stream()
    _, wp_b, _ = ops._pack(d, w, None, True, dev, st)
    rin = _amax_slot(ops, dy) if (arm and fam1 == 1) else None
    rout = _zslot(ops, dev)
    dx = torch.empty(B, Ci, Lx, device=dev)
    nb = L.lib.rh_conv1d_bwd_data_workspace_bytes(C.byref(d)) if use_ws else 0
    ws = _ws(ops, nb, dev) if nb > 0 else None
    L.lib.rh_x6_set_ranges(None, L.ptr(rin), L.ptr(rout), None)
    L.check(L.lib.rh_conv1d_bwd_data_f32(C.byref(d), L.ptr(dy), L.ptr(wp_b), L.ptr(x), None, L.ptr(add), L.ptr(dx), L.ptr(ws),
                                         nb, st), name)
    assert torch.isfinite(dx).all(), name
    _assert_publishes(rout, dx, f"dgrad {name} (family {fam1})")


def test_residual_unit_publishes_y_and_h(f16, dev):
    """rh_residual_unit_fwd_f32 (unit_x6.hip, one launch): the slots of y AND of the intermediate h."""
    ops = f16
    L = ops.L
    from rave_amd.ops import ConvGeom
    gen = torch.Generator().manual_seed(5)
    B, Cc, Lx = 3, 96, 515
    g3 = ConvGeom(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2)
    g1 = ConvGeom(act=1, slope=0.2)
    d3, d1 = ops._desc(g3, B, Cc, Cc, Lx, Lx, 3), ops._desc(g1, B, Cc, Cc, Lx, Lx, 1)
    assert L.lib.rh_residual_unit_fused(C.byref(d3), C.byref(d1)) == 1
    x = torch.randn(B, Cc, Lx, generator=gen) * 0.01
    x[-1, 7, -1] = -40.0                      # y's maximum is the residual term, negative, last column of the last item
    x = x.to(dev)
    w3 = (torch.randn(Cc, Cc, 3, generator=gen) / math.sqrt(3 * Cc)).to(dev)
    w1 = (torch.randn(Cc, Cc, 1, generator=gen) / math.sqrt(Cc)).to(dev)
    st = L.stream()
    wp3, _, _ = ops._pack(d3, w3, None, False, dev, st)
    wp1, _, _ = ops._pack(d1, w1, None, False, dev, st)
    rin, ry, rh = _amax_slot(ops, x), _zslot(ops, dev), _zslot(ops, dev)
    y, h = torch.empty_like(x), torch.empty_like(x)
    L.lib.rh_x6_set_ranges(None, L.ptr(rin), L.ptr(ry), L.ptr(rh))
    L.check(L.lib.rh_residual_unit_fwd_f32(C.byref(d3), C.byref(d1), L.ptr(x), L.ptr(wp3), L.ptr(wp1), L.ptr(h), L.ptr(y), st),
            "unit")
    _assert_publishes(ry, y, "unit y")
    _assert_publishes(rh, h, "unit h")


def test_act_bwd_bias_publishes_g(f16, dev):
    """rh_act_bwd_bias_f32 (conv_wgrad.hip): the slot of g = dy * act'(y), maximum in the last element, negative."""
    ops = f16
    L = ops.L
    gen = torch.Generator().manual_seed(6)
    B, M, plane = 3, 37, 1031
    dy = torch.randn(B, M, plane, generator=gen)
    y = torch.randn(B, M, plane, generator=gen)
    dy[-1, -1, -1], y[-1, -1, -1] = -500.0, 1.0
    dy, y = dy.to(dev), y.to(dev)
    g, db = torch.empty_like(dy), torch.empty(M, device=dev)
    nb = L.lib.rh_act_bwd_bias_workspace_bytes(M)
    ws = _ws(ops, nb, dev)
    rg = _zslot(ops, dev)
    L.lib.rh_x6_set_ranges(None, None, L.ptr(rg), None)
    L.check(L.lib.rh_act_bwd_bias_f32(L.ptr(dy), L.ptr(y), ops.ACT_LEAKY, 0.2, B, M, plane, L.ptr(g), L.ptr(db), L.ptr(ws), nb,
                                      L.stream()), "act_bwd_bias")
    _assert_publishes(rg, g, "act_bwd_bias g")


def _conv2d_family(ops, x, w, stride, padding):
    d = ops.L.Conv2dDesc(batch=x.shape[0], c_in=x.shape[1], c_out=w.shape[0], h_in=x.shape[2], w_in=x.shape[3],
                         h_out=(x.shape[2] + 2 * padding[0] - w.shape[2]) // stride[0] + 1,
                         w_out=(x.shape[3] + 2 * padding[1] - w.shape[3]) // stride[1] + 1,
                         kh=w.shape[2], kw=w.shape[3], sh=stride[0], sw=stride[1], dh=1, dw=1, ph=padding[0], pw=padding[1],
                         act=0, act_slope=0.0)
    info = (C.c_int64 * 16)()
    ops.L.check(ops.L.lib.rh_conv2d_plan_info(C.byref(d), 0, info), "conv2d_plan_info")
    return int(info[0])


@pytest.mark.parametrize("shape,x6", [((2, 32, 365, 5, 128, 5), True), ((3, 1, 401, 5, 32, 5), False)],
                         ids=["x6 period conv", "small-C first layer"])
def test_conv2d_forward_publishes_exactly_max_abs_y(f16, dev, shape, x6):
    ops = f16
    B, Ci, H, Wd, Co, kh = shape
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, H, Wd, generator=gen) * 0.01
    w = torch.randn(Co, Ci, kh, 1, generator=gen) / math.sqrt(Ci * kh)
    b = torch.randn(Co, generator=gen) * 0.01
    b[-1] = -200.0
    x, w, b = x.to(dev), w.to(dev), b.to(dev)
    fam = _conv2d_family(ops, x, w, (3, 1), (2, 0))
    assert (fam == 1) == x6, fam
    ops.range_reset(dev)
    with torch.no_grad():
        y = ops.conv2d(x, w, b, stride=(3, 1), padding=(2, 0))
    _assert_publishes(y._rh_range.slot, y, f"conv2d family {fam}")


def _conv2d_desc(ops, B, Ci, H, Wd, Co, kh, kw, sh, sw, ph, pw):
    return ops.L.Conv2dDesc(batch=B, c_in=Ci, c_out=Co, h_in=H, w_in=Wd, h_out=(H + 2 * ph - kh) // sh + 1,
                            w_out=(Wd + 2 * pw - kw) // sw + 1, kh=kh, kw=kw, sh=sh, sw=sw, dh=1, dw=1, ph=ph, pw=pw, act=0,
                            act_slope=0.0)


def test_conv2d_data_gradient_publishes_exactly_max_abs_dx(f16, dev):
    """rh_conv2d_bwd_data_f32 on the x6 kernel (conv2d_x6.hip, family 1): the slot of dx, maximum in the last element of the
    last batch item, negative."""
    ops = f16
    L = ops.L
    B, Ci, H, Wd, Co, kh = 2, 32, 365, 5, 128, 5
    d = _conv2d_desc(ops, B, Ci, H, Wd, Co, kh, 1, 3, 1, 2, 0)
    info = (C.c_int64 * 16)()
    L.check(L.lib.rh_conv2d_plan_info(C.byref(d), 1, info), "plan")
    assert int(info[0]) == 1
    gen = torch.Generator().manual_seed(9)
    w = (torch.randn(Co, Ci, kh, 1, generator=gen) / math.sqrt(Ci * kh)).to(dev)
    dy = torch.randn(B, Co, d.h_out, d.w_out, generator=gen) * 0.01
    dy[-1, -1, -1, -1] = -50.0
    dy = dy.to(dev)
    st = L.stream()
    wp_f = torch.empty(L.lib.rh_conv2d_packed_floats(C.byref(d), 0), device=dev)
    wp_b = torch.empty(L.lib.rh_conv2d_packed_floats(C.byref(d), 1), device=dev)
    L.check(L.lib.rh_conv2d_pack_f32(C.byref(d), L.ptr(w), L.ptr(wp_f), L.ptr(wp_b), st), "pack")
    rin, rout = _amax_slot(ops, dy), _zslot(ops, dev)
    dx = torch.empty(B, Ci, H, Wd, device=dev)
    L.lib.rh_x6_set_ranges(None, L.ptr(rin), L.ptr(rout), None)
    L.check(L.lib.rh_conv2d_bwd_data_f32(C.byref(d), L.ptr(dy), None, L.ptr(wp_b), L.ptr(dx), st), "conv2d dgrad")
    assert torch.isfinite(dx).all()
    _assert_publishes(rout, dx, "conv2d x6 dgrad")


def test_pqmf_analysis_and_reparametrize_publish(f16, dev):
    """The folded PQMF analysis kernel (pqmf_fold.hip) and the reparametrisation (misc.hip) publish their outputs' range."""
    ops = f16
    from rave_amd import pqmf
    m = pqmf.CachedPQMF(100, 16).to(dev)
    assert m._fold(m.forward_conv.weight) is not None         # the folded k1 kernel, not the direct form
    x = O.synthetic_batch(2, 1, 8192, seed=4).to(dev)
    x[-1, 0, -37:] = -3.0                     # a loud tail
    ops.range_reset(dev)
    with torch.no_grad():
        y = m(x)
        _assert_publishes(y._rh_range.slot, y, "pqmf fold k1")
        gen = torch.Generator().manual_seed(8)
        z = torch.randn(2, 32, 65, generator=gen)
        z[-1, 15, -1] = -90.0                 # a mean far out, negative, last element of the means
        eps = torch.randn(2, 16, 65, generator=gen)
        zs, _ = ops.reparametrize(z.to(dev), eps.to(dev))
        _assert_publishes(zs._rh_range.slot, zs, "reparametrize")
        # an edited bank takes the direct-form kernels, which publish nothing: the consumer's rh_amax_f32 pass fills the slot
        m.forward_conv.weight[3, 0, 200] += 1e-2
        assert m._fold(m.forward_conv.weight) is None
        y2 = m(x)
        assert getattr(y2, "_rh_range", None) is None
        _assert_publishes(ops._range_of(y2, ops.L.stream(), "pqmf direct"), y2, "pqmf direct form + rh_amax_f32")


@pytest.mark.parametrize("n", [1, 3, 5, 4097, 512 * 1024 * 4 + 7])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("where", ["first", "last", "body"])
def test_amax_direct(f16, dev, n, offset, where):
    """rh_amax_f32 (misc.hip: an unaligned head, a vector body, a tail) at odd base offsets and lengths."""
    ops = f16
    gen = torch.Generator().manual_seed(n + offset)
    buf = torch.rand(n + 4, generator=gen).to(dev)
    t = buf[offset:offset + n]
    pos = {"first": 0, "last": n - 1, "body": n // 2}[where]
    t[pos] = -7.5
    _assert_publishes(_amax_slot(ops, t), t, f"amax n={n} offset={offset} {where}")


@pytest.mark.parametrize("n", [5, 4097])
def test_amax_leaves_non_finite_elements_out(f16, dev, n):
    """The range of a tensor is the max |x| of its FINITE elements (common.hpp: rh_absmax): NaN and +-Inf are left out, so
    that an Inf element does not flush the rest of the tensor below the f16 pieces."""
    ops = f16
    t = torch.rand(n, generator=torch.Generator().manual_seed(n)).to(dev)
    t[n // 2] = -3.5
    ref = float(t.abs().max())
    t[0], t[n - 1], t[n // 3] = float("inf"), float("nan"), float("-inf")
    s = _amax_slot(ops, t)
    torch.cuda.synchronize()
    assert _smax(s) == ref


# --------------------------------------------------------------------------------------------------------------- B. consumer
def _x6_dilated(ops, dev):
    from rave_amd.ops import ConvGeom
    g = ConvGeom(dilation=3, pad_left=3, pad_right=3)
    return g


def _repr_error_var(x, scale_m):
    """Variance of the representation error of x (fp64) under the documented f16-piece scheme (common.hpp): scaled so that
    the tensor maximum sits in [2^14, 2^15), each element x' is held to h = max(2^-24 |x'|, 2^-25) -- round to nearest, so
    the error is uniform in [-h, h] (variance h^2 / 3), back in the original units h / scale."""
    e = math.floor(math.log2(scale_m)) if scale_m > 0 else -127
    scale = 2.0 ** min(14 - e, 125)
    h = torch.maximum(x.abs() * scale * 2.0 ** -24, torch.full_like(x, 2.0 ** -25)) / scale
    return h * h / 3.0


@pytest.mark.parametrize("quiet", [-16, -20, -24])
def test_quiet_clips_far_below_the_loud_one_meet_the_documented_window(f16, dev, quiet):
    """A batch whose clips span 2^0 ... 2^quiet in level: forward and data gradient of a k = 3 dilated conv on the f16 pieces,
    per clip, against fp64.  Bound: the input's representation error of the scheme (common.hpp:70-75) -- each element held to
    h = max(2^-24 |x'|, 2^-25) of the scaled x' (the tensor maximum in [2^14, 2^15)), rounding error uniform in [-h, h] --
    propagated through the conv in fp64 (var(dy) = conv(var(dx), w^2), independent errors) as the predicted error norm E of each
    clip; the measured error must stay below 1.4 E plus the f32 class of the loud clips (16 * 2^-24 of the clip's norm).  A window
    one bit narrower doubles E on the quiet clips (where the 2^-25 floor dominates) and fails.  The weight gradient (dominated by
    the loud clips) is checked at the f32 class."""
    ops = f16
    g = _x6_dilated(ops, dev)
    gen = torch.Generator().manual_seed(21 - quiet)
    B, Cc, Lx = 4, 96, 2048
    levels = torch.tensor([1.0, 2.0 ** (quiet // 2), 2.0 ** quiet, 0.5], dtype=torch.float64).view(B, 1, 1)
    x = (torch.randn(B, Cc, Lx, generator=gen, dtype=torch.float64) * levels).float()
    cot = (torch.randn(B, Cc, Lx, generator=gen, dtype=torch.float64) * levels).float()
    w = torch.randn(Cc, Cc, 3, generator=gen) / (3 * Cc) ** 0.5
    d = ops._desc(g, B, Cc, Cc, Lx, Lx, 3)
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 0, 0, 0) == 1
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 1, 0, 0) == 1
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    ops.range_reset(dev)
    y = ops.conv1d(xd, wd, geom=g)
    gx, gw = torch.autograd.grad(y, (xd, wd), cot.to(dev))
    x64, w64, c64 = x.double().requires_grad_(True), w.double().requires_grad_(True), cot.double()
    y64 = F.conv1d(x64, w64, padding=3, dilation=3)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), c64)
    # predicted representation error of each clip's output (forward: x's pieces; data gradient: dy's pieces, transposed conv)
    var_y = F.conv1d(_repr_error_var(x.double(), float(x.abs().max())), w.double() ** 2, padding=3, dilation=3)
    var_gx = F.conv_transpose1d(_repr_error_var(cot.double(), float(cot.abs().max())), w.double() ** 2, padding=3, dilation=3)
    worst = 0.0
    for b in range(B):
        for what, got, ref, var in (("y", y.detach()[b], y64[b], var_y[b]), ("dx", gx[b], gx64[b], var_gx[b])):
            err = float((got.cpu().double() - ref.detach()).norm())
            e_pred = float(var.sum().sqrt())
            bound = 1.4 * e_pred + 16 * 2.0 ** -24 * float(ref.detach().norm())
            worst = max(worst, err / bound)
            assert err <= bound, (what, b, float(levels[b]), err, e_pred, bound)
    assert rel_l2(gw.cpu().double(), gw64) < 2e-6
    print(f"clips down to 2^{quiet}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["zero", "impulse", "huge", "tiny", "subnormal"])
def test_whole_tensor_edges_of_the_scale_scheme(f16, dev, kind):
    """Forward, data gradient and weight gradient of the x6 k = 3 dilated conv against fp64 for tensors at the edges of the
    scale scheme.  zero: exactly zero (the bias exactly, forward); impulse: the weight taps to f32 rounding; huge (max ~2^100):
    finite and f32-accurate; tiny (max below 2^-111, the clamp of common.hpp: scaled by 2^125 only) and f32 subnormals: finite
    and held to max(2^-24 |x|, 2^-150) per element, i.e. f32-accurate."""
    ops = f16
    g = _x6_dilated(ops, dev)
    gen = torch.Generator().manual_seed(33)
    B, Cc, Lx = 2, 96, 300
    w = torch.randn(Cc, Cc, 3, generator=gen) / (3 * Cc) ** 0.5
    bias = torch.randn(Cc, generator=gen)
    base = torch.randn(B, Cc, Lx, generator=gen)
    if kind == "zero":
        x = torch.zeros(B, Cc, Lx)
    elif kind == "impulse":
        x = torch.zeros(B, Cc, Lx)
        x[1, 5, 100] = 1.0
    elif kind == "huge":
        x = base * 2.0 ** 100
    elif kind == "tiny":
        x = base * 2.0 ** -115
    else:
        x = base * 2.0 ** -135           # f32 subnormals (min normal 2^-126)
        assert (x[x != 0].abs() < 2.0 ** -126).all()
    # the weight scale for "huge": keep y finite in f32 (~2^100 * 5); cotangent of a moderate size
    cot = torch.randn(B, Cc, Lx, generator=gen)
    d = ops._desc(g, B, Cc, Cc, Lx, Lx, 3)
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 0, 1, 0) == 1
    xd, wd, bd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), bias.to(dev)
    ops.range_reset(dev)
    y = ops.conv1d(xd, wd, bd, geom=g)
    y0 = ops.conv1d(xd, wd, geom=g)
    gx, gw = torch.autograd.grad(y0, (xd, wd), cot.to(dev))
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv1d(x64, w64, padding=3, dilation=3)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), cot.double())
    y, y0 = y.detach().cpu(), y0.detach().cpu()
    for t in (y, y0, gx, gw):
        assert torch.isfinite(t).all(), kind
    if kind == "zero":
        assert torch.equal(y0, torch.zeros_like(y0))
        assert torch.equal(y, bias.view(1, -1, 1).expand_as(y))
        assert torch.equal(gw.cpu(), torch.zeros_like(gw.cpu()))
        return
    if kind == "impulse":
        # y[b, :, 100 - 3 (t - 1)] = w[:, 5, t]: the taps themselves, to f32 rounding
        for t in range(3):
            assert torch.allclose(y0[1, :, 100 + 3 * (1 - t)], w[:, 5, t], rtol=2 ** -22, atol=0), t
        assert torch.equal(y0[0], torch.zeros_like(y0[0]))
    # f32 class against fp64 (subnormal operands: their products sit near the bottom of f32, an absolute floor of 2^-149 per
    # output element on top)
    floor = 2.0 ** -149 * math.sqrt(y64.numel()) * 8 if kind in ("tiny", "subnormal") else 0.0
    for what, got, ref in (("y", y0, y64), ("dx", gx, gx64), ("dw", gw, gw64)):
        err = float((got.cpu().double() - ref.detach()).norm())
        assert err <= 2e-6 * float(ref.detach().norm()) + floor, (kind, what, err, float(ref.detach().norm()))


def test_weight_rows_spanning_twenty_octaves(f16, dev):
    """Weight rows at 2^0 ... 2^-20 of the largest row.  The packers record ONE range per weight tensor (the per-row max |w| of
    rh_prep_fill_item / the pack kernels is reduced to the tensor's maximum, the word the f16 kernels scale by), so a quiet row
    is held to the tensor's window: each element to max(2^-24 |w'|, 2^-25) of the scaled w' (maximum in [2^14, 2^15)).  Per
    output channel against fp64: the error must stay below 1.4 x the prediction of that representation (var(dy) =
    conv(x^2, var(dw)), fp64) plus the f32 class (16 * 2^-24 of the channel's norm)."""
    ops = f16
    g = _x6_dilated(ops, dev)
    gen = torch.Generator().manual_seed(44)
    B, Cc, Lx = 2, 96, 512
    rows = 2.0 ** -(torch.arange(Cc) % 21).double()
    w = (torch.randn(Cc, Cc, 3, generator=gen, dtype=torch.float64) / (3 * Cc) ** 0.5 * rows.view(-1, 1, 1)).float()
    x = torch.randn(B, Cc, Lx, generator=gen)
    d = ops._desc(g, B, Cc, Cc, Lx, Lx, 3)
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 0, 0, 0) == 1
    ops.range_reset(dev)
    with torch.no_grad():
        y = ops.conv1d(x.to(dev), w.to(dev), geom=g).cpu().double()
    y64 = F.conv1d(x.double(), w.double(), padding=3, dilation=3)
    var = F.conv1d(x.double() ** 2, _repr_error_var(w.double(), float(w.abs().max())), padding=3, dilation=3)
    worst = 0.0
    for c in range(Cc):
        err = float((y[:, c] - y64[:, c]).norm())
        bound = 1.4 * float(var[:, c].sum().sqrt()) + 16 * 2.0 ** -24 * float(y64[:, c].norm())
        worst = max(worst, err / bound)
        assert err <= bound, (c, float(rows[c]), err, bound)
    print(f"weight rows down to 2^-20: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["quiet", "huge", "tiny", "subnormal"])
def test_conv2d_x6_at_the_edges_of_the_scale_scheme(f16, dev, kind):
    """The 2-D f16-piece kernels (conv2d_x6.hip forward and data gradient, wgrad2d_x6.hip weight gradient; all family 1 at this
    shape) against fp64 F.conv2d.  quiet: batch items at 2^0 and 2^-20, each item's forward / data-gradient error below 1.4 x
    the prediction of the documented representation (as the 1-D test) plus the f32 class; huge (max ~2^100): f32-accurate;
    tiny (max below 2^-111) and f32 subnormals: f32-accurate with the 2^-149 floor of f32 itself (the unscale of quiet
    products is a subnormal power of two, common.hpp: rh_x6_unscale_bits)."""
    ops = f16
    L = ops.L
    B, Ci, H, Wd, Co, kh = 2, 32, 96, 6, 32, 5
    d = _conv2d_desc(ops, B, Ci, H, Wd, Co, kh, 1, 1, 1, 2, 0)
    for which in (0, 1):
        info = (C.c_int64 * 16)()
        L.check(L.lib.rh_conv2d_plan_info(C.byref(d), which, info), "plan")
        assert int(info[0]) == 1, which
    assert L.lib.rh_conv2d_bwd_weight_kernel_family(C.byref(d)) == 1
    gen = torch.Generator().manual_seed(66)
    w = torch.randn(Co, Ci, kh, 1, generator=gen) / math.sqrt(Ci * kh)
    base = torch.randn(B, Ci, H, Wd, generator=gen, dtype=torch.float64)
    cot = torch.randn(B, Co, H, Wd, generator=gen, dtype=torch.float64)
    if kind == "quiet":
        lv = torch.tensor([1.0, 2.0 ** -20], dtype=torch.float64).view(B, 1, 1, 1)
        x, cot = (base * lv).float(), (cot * lv).float()
    else:
        x = (base * {"huge": 2.0 ** 100, "tiny": 2.0 ** -115, "subnormal": 2.0 ** -135}[kind]).float()
        cot = cot.float()
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    ops.range_reset(dev)
    y = ops.conv2d(xd, wd, stride=1, padding=(2, 0))
    gx, gw = torch.autograd.grad(y, (xd, wd), cot.to(dev))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, padding=(2, 0))
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), cot.double())
    outs = (("y", y.detach().cpu().double(), y64.detach()), ("dx", gx.cpu().double(), gx64), ("dw", gw.cpu().double(), gw64))
    for what, got, ref in outs:
        assert torch.isfinite(got).all(), (kind, what)
    if kind == "quiet":
        var_y = F.conv2d(_repr_error_var(x.double(), float(x.abs().max())), w.double() ** 2, padding=(2, 0))
        var_gx = F.conv_transpose2d(_repr_error_var(cot.double(), float(cot.abs().max())), w.double() ** 2, padding=(2, 0))
        for b in range(B):
            for what, got, ref, var in (("y", outs[0][1][b], y64[b].detach(), var_y[b]), ("dx", outs[1][1][b], gx64[b], var_gx[b])):
                err = float((got - ref).norm())
                bound = 1.4 * float(var.sum().sqrt()) + 16 * 2.0 ** -24 * float(ref.norm())
                assert err <= bound, (what, b, err, bound)
        assert rel_l2(outs[2][1], gw64) < 2e-6
        return
    for what, got, ref in outs:
        floor = 2.0 ** -149 * math.sqrt(ref.numel()) * 8 if kind in ("tiny", "subnormal") else 0.0
        err = float((got - ref).norm())
        assert err <= 2e-6 * float(ref.norm()) + floor, (kind, what, err, float(ref.norm()))


def test_weight_norm_batched_packer_records_the_range_of_the_normalised_weight(f16, dev):
    """The batched weight-norm packer (rave_amd.prep.WeightPrep -> rh_prep_fill_item / rh_prep_run_f32: w = g v / ||v||, the
    per-row max |w| and sum |w| reduced to the tensor's range record) with rows at 2^0 ... 2^-20: the same per-channel bound
    as the plain packer's (the window of the normalised weight's maximum), against fp64 of g v / ||v||."""
    ops = f16
    from rave_amd import blocks, cc, prep
    g = _x6_dilated(ops, dev)
    gen = torch.Generator().manual_seed(45)
    B, Cc, Lx = 2, 96, 512
    conv = blocks.normalization(cc.Conv1d(Cc, Cc, 3, padding=(3, 3), dilation=3, bias=False), "weight_norm")
    rows = 2.0 ** -(torch.arange(Cc) % 21).double()
    v = torch.randn(Cc, Cc, 3, generator=gen, dtype=torch.float64)
    gains = (rows * 0.3).view(-1, 1, 1)
    with torch.no_grad():
        conv.weight_v.copy_(v.float())
        conv.weight_g.copy_(gains.float())
    conv = conv.to(dev)
    wv, wg = conv.weight_v.detach().cpu().double(), conv.weight_g.detach().cpu().double()
    w64 = wg * wv / wv.norm(dim=(1, 2), keepdim=True)
    x = torch.randn(B, Cc, Lx, generator=gen)
    d = ops._desc(g, B, Cc, Cc, Lx, Lx, 3)
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 0, 0, 0) == 1
    wp = prep.WeightPrep(torch.nn.Sequential(conv))
    assert wp.n == 1
    ops.range_reset(dev)
    wp.run()
    try:
        assert getattr(conv, "_prepacked", None) is not None
        with torch.no_grad():
            y = conv(x.to(dev)).cpu().double()
    finally:
        wp.release()
    y64 = F.conv1d(x.double(), w64, padding=3, dilation=3)
    var = F.conv1d(x.double() ** 2, _repr_error_var(w64, float(w64.abs().max())), padding=3, dilation=3)
    for c in range(Cc):
        err = float((y[:, c] - y64[:, c]).norm())
        bound = 1.4 * float(var[:, c].sum().sqrt()) + 16 * 2.0 ** -24 * float(y64[:, c].norm())
        assert err <= bound, (c, float(rows[c]), err, bound)


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_non_finite_inputs_stay_where_fp64_puts_them(f16, dev, bad):
    """A NaN / Inf in x: non-finite outputs at exactly the positions where the fp64 reference is non-finite, finite and
    f32-accurate everywhere else (the values AT those positions are not asserted: hi - lo of an Inf is NaN).  Also through a
    producer: the same x as the output of an x6 conv (whose published slot must leave the Inf out) feeding a second one."""
    ops = f16
    g = _x6_dilated(ops, dev)
    gen = torch.Generator().manual_seed(55)
    B, Cc, Lx = 2, 96, 300
    w = torch.randn(Cc, Cc, 3, generator=gen) / (3 * Cc) ** 0.5
    x = torch.randn(B, Cc, Lx, generator=gen)
    x[1, 40, 150] = float(bad)
    ops.range_reset(dev)
    with torch.no_grad():
        y = ops.conv1d(x.to(dev), w.to(dev), geom=g).cpu()
    y64 = F.conv1d(x.double(), w.double(), padding=3, dilation=3)
    fin = torch.isfinite(y64)
    assert torch.equal(torch.isfinite(y), fin)
    assert rel_l2(y[fin], y64[fin]) < 2e-6
    # the non-finite value produced by a conv (residual term of a k = 1 identity-free conv: y1 = conv(x0) + r, r holding it)
    r = torch.zeros(B, Cc, Lx)
    r[1, 40, 150] = float(bad)
    x0 = torch.randn(B, Cc, Lx, generator=gen)
    w0 = torch.randn(Cc, Cc, 3, generator=gen) / (3 * Cc) ** 0.5
    with torch.no_grad():
        y1 = ops.conv1d(x0.to(dev), w0.to(dev), geom=g, residual=r.to(dev))
        torch.cuda.synchronize()
        if bad != "nan":
            assert _smax(y1._rh_range.slot) == float(y1[torch.isfinite(y1)].abs().max())
        y = ops.conv1d(y1, w.to(dev), geom=g).cpu()
    x1 = F.conv1d(x0.double(), w0.double(), padding=3, dilation=3) + r.double()
    y64 = F.conv1d(x1, w.double(), padding=3, dilation=3)
    fin = torch.isfinite(y64)
    assert torch.equal(torch.isfinite(y), fin)
    assert rel_l2(y[fin], y64[fin]) < 2e-6


# --------------------------------------------------------------------------------------------------------------- C. lifetime
def _x6_geom():
    from rave_amd.ops import ConvGeom
    return ConvGeom(dilation=1, pad_left=1, pad_right=1, act=1, slope=0.2)


def _chain_operands(dev, seed=61):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 96, 1024, generator=gen).to(dev)
    w1 = (torch.randn(96, 96, 3, generator=gen) / 17).to(dev)
    w2 = (torch.randn(96, 96, 3, generator=gen) / 17).to(dev)
    return x, w1, w2


def _small_model(dev):
    from rave_amd import model as M
    torch.manual_seed(0)
    m = M.build_v2(capacity=16, latent_size=16).to(dev).train()
    m.configure_optimizers(capturable=True)
    return m


def test_eager_work_around_a_recorded_step_never_uses_the_graphs_slots(f16, dev):
    """After GraphedTrainingStep records a step, the slot pool the recording took belongs to the graph: every replay re-zeroes
    it, and before the first replay it was never zeroed.  Eager x6 convs before / after a capture and across a replay must give
    the results of the same chain in a process state without any capture, bit for bit; and so must decode(encode(x)) with a
    replayed step in between."""
    ops = f16
    from rave_amd import model as M
    g = _x6_geom()
    x, w1, w2 = _chain_operands(dev)
    d = ops._desc(g, 2, 96, 96, 1024, 1024, 3)
    assert ops.L.lib.rh_conv1d_kernel_family(C.byref(d), 0, 0, 0) == 1

    def chain_first():
        with torch.no_grad():
            return ops.conv1d(x, w1, geom=g)

    def chain_second(y):
        with torch.no_grad():
            return ops.conv1d(y, w2, geom=g)

    ops.range_reset(dev)
    ref = chain_second(chain_first())
    m = _small_model(dev)
    other = _small_model(dev)          # eager encode / decode on a second model: its parameters do not move with the replays
    xb = O.synthetic_batch(2, 1, 32768, seed=62).to(dev)
    eps = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    def encode(xb):           # z = the reparametrised latent (its slot published by the reparametrisation kernel)
        return other.encoder.reparametrize(other.encode(xb), eps)[0]

    with torch.no_grad():
        z_ref = encode(xb)
        dec_ref = other.decode(z_ref)
    step = M.GraphedTrainingStep(m, xb, inject_eps=True)
    # (1) recorded, nothing replayed yet: produce y eagerly and consume it
    step.capture(xb, 0, eps=eps)
    y = chain_first()
    out1 = chain_second(y)
    assert torch.isfinite(out1).all()
    assert torch.equal(out1, ref)
    # (2) y produced eagerly, one replay, then consumed; z = encode(x), one replay, decode(z)
    y = chain_first()
    with torch.no_grad():
        z = encode(xb)
    step(xb, 0, eps=eps)
    torch.cuda.synchronize()
    out2 = chain_second(y)
    with torch.no_grad():
        dec = other.decode(z)
    assert torch.isfinite(out2).all() and torch.isfinite(dec).all()
    assert torch.equal(out2, ref)
    assert torch.equal(z, z_ref)
    assert torch.equal(dec, dec_ref)
    assert key_pools(step) > 0


def key_pools(step) -> int:
    """The pools each recorded graph owns (kept alive with it)."""
    return sum(len(v) for v in step.range_pools.values())


def test_a_pool_taken_inside_a_raw_capture_is_not_handed_out_eagerly(f16, dev):
    """A caller that records its own graph (range_reset inside torch.cuda.graph, as bench.py does) without range_capture_end:
    the next eager slot still comes from a fresh pool, not from the one the graph owns."""
    ops = f16
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.range_reset(dev)
    owned = ops._RANGE_POOLS[dev].pool
    assert ops._RANGE_POOLS[dev].captured
    slot = ops._new_range(dev)
    assert slot.untyped_storage().data_ptr() != owned.untyped_storage().data_ptr()
    assert not ops._RANGE_POOLS[dev].captured
    del g


def test_version_counters_and_views(f16, dev):
    """In-place writes invalidate a slot (the consumer's result stays right); a view / reshape of the whole output reuses the
    producer's slot (no rh_amax_f32 pass); a partial slice gets a slot of its own that covers it."""
    ops = f16
    g = _x6_geom()
    x, w1, w2 = _chain_operands(dev, 63)
    ops.range_reset(dev)

    def consume(t):
        with torch.no_grad():
            return ops.conv1d(t, w2, geom=g)

    def ref(t):
        return F.conv1d(F.leaky_relu(t.double().cpu(), 0.2), w2.double().cpu(), padding=1)

    with torch.no_grad():
        y = ops.conv1d(x, w1, geom=g)
    slot = y._rh_range.slot
    y.mul_(2.0 ** 20)
    out = consume(y)
    assert torch.isfinite(out).all() and rel_l2(out, ref(y)) < 2e-6
    y[0, 0, -1] = 1e6 * 2.0 ** 20
    out = consume(y)
    assert torch.isfinite(out).all() and rel_l2(out, ref(y)) < 2e-6
    assert _smax(y._rh_range.slot) == float(y.abs().max())
    # a view of the whole output: the producer's slot, no pass
    with torch.no_grad():
        y = ops.conv1d(x, w1, geom=g)
    slot = y._rh_range.slot
    ops.range_miss_log_begin()
    v = y.view(2, 96, 1024)
    consume(v)
    consume(y.reshape(2, 96, 1024))
    assert ops.range_miss_log_end() == []
    assert v._rh_range.slot.data_ptr() == slot.data_ptr()
    # a partial slice: its own slot, which covers it
    part = y[1:]
    ops.range_miss_log_begin()
    out = consume(part)
    miss = ops.range_miss_log_end()
    assert len(miss) == 1
    assert part._rh_range.slot.data_ptr() != slot.data_ptr()
    torch.cuda.synchronize()
    assert _smax(part._rh_range.slot) == float(part.abs().max())
    assert rel_l2(out, ref(part)) < 2e-6


def test_slot_filled_on_the_side_stream_is_ordered_before_a_compute_stream_reader(f16, dev):
    """A slot rh_amax_f32 filled on the weight-gradient side stream (ops._wgrad_ranges under _OnSide) must not be read on
    the compute stream before that pass has run: a sleep queued on the side stream ahead of the pass makes the race
    deterministic, and the compute-stream consumer must still equal the single-stream result."""
    ops = f16
    g = _x6_geom()
    x, w1, _ = _chain_operands(dev, 64)
    ops.range_reset(dev)
    with torch.no_grad():
        ref = ops.conv1d(x.clone(), w1, geom=g)          # (a fresh tensor: its slot on the compute stream)
        t = x.clone()                                    # no slot yet
        torch.cuda.synchronize()
        side = ops._side_stream(dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.cuda._sleep(200_000_000)               # ~0.1 s of side-stream work ahead of the pass
            ops._range_of(t, ops.L.stream(), "side")
        out = ops.conv1d(t, w1, geom=g)                  # compute stream: reads t's slot
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)


def test_pool_exhaustion_in_the_middle_of_a_step_is_bit_identical(f16, dev, monkeypatch):
    """A slot pool that runs out in the middle of an eager training step (full width, batch 2, weight gradients on the side
    stream) is replaced (ops.range_reset(_exhausted=True): the other stream waits for the new pool's zero fill).  With a pool of a
    handful of slots the step must land bit for bit where it lands with the default pool, and the replacement must have
    happened while the side stream was in use."""
    ops = f16
    from rave_amd import _ranges, model as M
    xb = O.synthetic_batch(2, 1, 32768, seed=65).to(dev)
    eps = torch.randn(2, 128, 16, generator=torch.Generator().manual_seed(4)).to(dev)

    def step():
        torch.manual_seed(0)
        m = M.build_v2().to(dev).train()
        m.configure_optimizers()
        logged = m.training_step(xb.clone(), 0, eps=eps)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.named_parameters()}, {k: float(v) for k, v in logged.items()}

    p_ref, l_ref = step()
    seen = []
    orig = _ranges.range_reset

    def spy(device=None, _exhausted=False):
        if _exhausted:
            d_ = device if isinstance(device, torch.device) else torch.device(device)
            side = ops.SIDE.streams.get(d_.index if d_.index is not None else torch.cuda.current_device())
            # (a weight-gradient branch forked and not yet joined: the side stream is working beside this replacement)
            seen.append((ops.SIDE.pending is not None, side is not None and torch.cuda.current_stream(d_) == side))
        return orig(device, _exhausted)

    monkeypatch.setattr(_ranges, "_RANGE_SLOTS", 5)       # (where _new_range looks both up)
    monkeypatch.setattr(_ranges, "range_reset", spy)
    ops._RANGE_POOLS.clear()
    p, lg = step()
    monkeypatch.undo()
    ops._RANGE_POOLS.clear()
    # replaced many times, some of them while a weight-gradient branch was running on the side stream (then the new pool's
    # zero fill must be waited for across the streams)
    assert len(seen) > 10 and any(e for e, _ in seen), seen[:20]
    print(f"{len(seen)} pool replacements, {sum(o for _, o in seen)} of them on the side stream")
    assert lg == l_ref
    for k in p_ref:
        assert torch.equal(p[k], p_ref[k]), k


# --------------------------------------------------------------------------------------------------------------- D. armed state
def _unit_descs(ops, B=2, Cc=96, Lx=256):
    from rave_amd.ops import ConvGeom
    g3 = ConvGeom(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2)
    g1 = ConvGeom(act=1, slope=0.2)
    return ops._desc(g3, B, Cc, Cc, Lx, Lx, 3), ops._desc(g1, B, Cc, Cc, Lx, Lx, 1)


FAILING_CALLS = ["conv1d_fwd", "conv1d_bwd_data", "residual_unit_fwd", "residual_unit_unfusable", "conv1d_bwd_weight",
                 "conv1d_bwd_weight_wn", "conv2d_fwd", "act_bwd_bias", "reparam_fwd", "pqmf_fold_k1"]


def _failing_call(ops, which, d3, d1):
    """One call of each entry point that consumes the armed slots, made to fail validation (null pointers / bad sizes)."""
    L = ops.L
    lib, st = L.lib, L.stream()
    r3, r1 = C.byref(d3), C.byref(d1)
    if which == "conv1d_fwd":
        return lib.rh_conv1d_fwd_f32(r3, None, None, None, None, None, None, None, 0, st)
    if which == "conv1d_bwd_data":
        return lib.rh_conv1d_bwd_data_f32(r3, None, None, None, None, None, None, None, 0, st)
    if which == "residual_unit_fwd":
        return lib.rh_residual_unit_fwd_f32(r3, r1, None, None, None, None, None, st)
    if which == "residual_unit_unfusable":
        return lib.rh_residual_unit_fwd_f32(r1, r3, None, None, None, None, None, st)
    if which == "conv1d_bwd_weight":
        return lib.rh_conv1d_bwd_weight_f32(r3, None, None, None, None, None, None, 0, st)
    if which == "conv1d_bwd_weight_wn":
        return lib.rh_conv1d_bwd_weight_wn_f32(r3, None, None, None, None, None, None, None, None, None, None, None, 0, st)
    if which == "conv2d_fwd":
        d2 = L.Conv2dDesc(batch=1, c_in=32, c_out=32, h_in=8, w_in=1, h_out=8, w_out=1, kh=1, kw=1, sh=1, sw=1, dh=1, dw=1,
                          ph=0, pw=0, act=0, act_slope=0.0)
        return lib.rh_conv2d_fwd_f32(C.byref(d2), None, None, None, None, st)
    if which == "act_bwd_bias":
        return lib.rh_act_bwd_bias_f32(None, None, 0, 0.0, 1, 1, 1, None, None, None, 0, st)
    if which == "reparam_fwd":
        return lib.rh_reparam_fwd_f32(None, None, 1, 1, 1, None, None, None, 0, st)
    if which == "pqmf_fold_k1":
        return lib.rh_pqmf_fold_k1_f32(None, None, 1, 16, 1, 0, 1.0, None, st)
    raise AssertionError(which)


@pytest.mark.parametrize("which", FAILING_CALLS)
def test_armed_slots_are_consumed_by_a_failing_call(f16, dev, which):
    """Arm a zero input slot and an output buffer, make a call that fails validation, then run a valid UNARMED x6-eligible conv:
    the buffer stays zero, and the conv takes the f32-input kernels (finite, f32-accurate against fp64) instead of reading the
    stale zero slot (scale 2^125: Inf)."""
    ops = f16
    L = ops.L
    d3, d1 = _unit_descs(ops)
    zero_in = _zslot(ops, dev)
    out, out2 = _zslot(ops, dev), _zslot(ops, dev)
    torch.cuda.synchronize()
    L.lib.rh_x6_set_ranges(L.ptr(zero_in), L.ptr(zero_in), L.ptr(out), L.ptr(out2))
    rc = _failing_call(ops, which, d3, d1)
    assert rc in (-1, -2), (which, rc)
    # the next, unrelated call: a valid x6-eligible forward without any slot armed
    gen = torch.Generator().manual_seed(71)
    x = torch.randn(2, 96, 256, generator=gen)
    w = torch.randn(96, 96, 3, generator=gen) / 17
    assert L.lib.rh_conv1d_kernel_family(C.byref(d3), 0, 0, 0) == 1
    xd = x.to(dev)
    wp, _, _ = ops._pack(d3, w.to(dev), None, False, dev, L.stream())
    y = torch.empty_like(xd)
    nb = L.lib.rh_conv1d_fwd_workspace_bytes(C.byref(d3))
    ws = _ws(ops, nb, dev)
    L.check(L.lib.rh_conv1d_fwd_f32(C.byref(d3), L.ptr(xd), L.ptr(wp), None, None, None, L.ptr(y), L.ptr(ws), nb, L.stream()),
            "valid conv")
    torch.cuda.synchronize()
    assert int(out.abs().max()) == 0 and int(out2.abs().max()) == 0, which
    assert torch.isfinite(y).all(), which
    y64 = F.conv1d(F.leaky_relu(x.double(), 0.2), w.double(), padding=3, dilation=3)
    assert rel_l2(y.cpu().double(), y64) < 2e-6, which


def _raise_in_conv1d_fwd(ops, dev, x):
    xs = x * 2.0 ** -40                 # (armed: an input slot 2^40 too small for x below)
    ops._range_of(xs, ops.L.stream(), "xs")
    return lambda: ops.conv1d(xs, _chain_operands(dev, 74)[1], geom=_x6_geom())


def _raise_in_act_bwd_bias(ops, dev, x):
    """conv2d with a bias and an output LeakyReLU, backward: (B, C_out, plane) of test_act_bwd_bias_publishes_g."""
    gen = torch.Generator().manual_seed(75)
    x2 = torch.randn(3, 4, 1031, 1, generator=gen).to(dev)
    w = (torch.randn(37, 4, 3, 1, generator=gen) / 4).to(dev).requires_grad_(True)
    b = torch.randn(37, generator=gen).to(dev).requires_grad_(True)
    y = ops.conv2d(x2, w, b, padding=(1, 0), act=ops.ACT_LEAKY, slope=0.2)
    assert tuple(y.shape) == (3, 37, 1031, 1)
    return lambda: y.sum().backward()


def _raise_in_pqmf_fold_k1(ops, dev, x):
    from rave_amd import pqmf
    m = pqmf.CachedPQMF(100, 16).to(dev)
    assert m._fold(m.forward_conv.weight) is not None         # the folded k1 kernel, not the direct form
    xw = O.synthetic_batch(2, 1, 8192, seed=4).to(dev)
    return lambda: m(xw)


def _raise_in_reparam_fwd(ops, dev, x):
    gen = torch.Generator().manual_seed(8)
    z, eps = torch.randn(2, 32, 65, generator=gen).to(dev), torch.randn(2, 16, 65, generator=gen).to(dev)
    return lambda: ops.reparametrize(z, eps)


def _raise_in_profiled_conv1d_fwd(ops, dev, x):
    ops._range_of(x, ops.L.stream(), "x")
    w1 = _chain_operands(dev, 74)[1]

    def call():
        ops.profile_begin()
        ops.conv1d(x, w1, geom=_x6_geom())
    return call


class _OnBackwardThread(torch.autograd.Function):
    """Runs ``fn`` where autograd runs the backward of GPU nodes: a thread of its own, and the armed state is thread-local."""

    @staticmethod
    def forward(ctx, t, fn):
        ctx.fn = fn
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


# (name, entry point made to raise, preparation -> the failing call, in backward): the first is the guarded 1-D forward, the others
# the sites that armed without a guard before rave_amd/_arming.py (the three publishers of an out-slot, and the kernel events
# of a profiled launch)
RAISING_SITES = [
    ("conv1d forward", "rh_conv1d_fwd_f32", _raise_in_conv1d_fwd, False),
    ("conv2d backward act_bwd_bias", "rh_act_bwd_bias_f32", _raise_in_act_bwd_bias, True),
    ("pqmf analysis folded", "rh_pqmf_fold_k1_f32", _raise_in_pqmf_fold_k1, False),
    ("reparametrize", "rh_reparam_fwd_f32", _raise_in_reparam_fwd, False),
    ("profiled conv1d forward", "rh_conv1d_fwd_f32", _raise_in_profiled_conv1d_fwd, False),
]


@pytest.mark.parametrize("site", RAISING_SITES, ids=[c[0] for c in RAISING_SITES])
def test_python_side_disarms_when_the_call_raises(f16, dev, monkeypatch, site):
    """ops arms the slots (a profiled launch: also the kernel events) of a call and then calls the library; if that call raises
    in Python (here: the entry point itself), the armed state is dropped and cannot reach the next call of the thread: an
    unrelated, unarmed 1-D forward stays f32-accurate (an in-slot left armed: 2^40 too small), publishes nothing into the
    freshly reset pool (an out-slot left armed: the slot the failing call had taken from it) and takes no kernel events."""
    ops = f16
    L = ops.L
    name, entry, prepare, in_backward = site
    g = _x6_geom()
    x, w1, _ = _chain_operands(dev, 74)

    def boom(*a):
        raise RuntimeError("injected")

    d3 = ops._desc(g, 2, 96, 96, 1024, 1024, 3)
    wp, _, _ = ops._pack(d3, w1, None, False, dev, L.stream())
    failing = prepare(ops, dev, x)          # (whatever needs a slot has taken it from the pool before this one)
    ops.range_reset(dev)
    pool = ops._RANGE_POOLS[dev].pool
    monkeypatch.setattr(L.lib, entry, boom)
    with pytest.raises(RuntimeError, match="injected"), torch.set_grad_enabled(in_backward):
        failing()
    monkeypatch.undo()
    y = torch.empty_like(x)
    events_used = []

    def unrelated():
        L.check(L.lib.rh_conv1d_fwd_f32(C.byref(d3), L.ptr(x), L.ptr(wp), None, None, None, L.ptr(y), None, 0, L.stream()), "conv")
        events_used.append(L.lib.rh_kernel_events_used())

    if in_backward:         # (the next call of the thread that armed)
        _OnBackwardThread.apply(torch.zeros(1, device=dev, requires_grad=True), unrelated).sum().backward()
    else:
        unrelated()
    torch.cuda.synchronize()
    ref = F.conv1d(F.leaky_relu(x.double().cpu(), 0.2), w1.double().cpu(), padding=1)
    assert torch.isfinite(y).all()
    assert rel_l2(y.cpu().double(), ref) < 2e-6
    assert int(pool.abs().max()) == 0
    assert events_used == [0]


def _wgrad_operands(ops, dev):
    from rave_amd.ops import ConvGeom
    gen = torch.Generator().manual_seed(72)
    B, Cc, Lx = 8, 96, 4096
    g = ConvGeom(dilation=1, pad_left=1, pad_right=1)
    d = ops._desc(g, B, Cc, Cc, Lx, Lx, 3)
    x = torch.randn(B, Cc, Lx, generator=gen)
    dy = torch.randn(B, Cc, Lx, generator=gen)
    return d, x, dy


def test_armed_defer_is_consumed_by_a_failing_weight_gradient(f16, dev):
    """rh_defer_reduce(item) then a FAILING rh_conv1d_bwd_weight_f32: the next valid weight gradient of a K-split shape must
    return a fully reduced dw (fp64) and leave the item untouched."""
    ops = f16
    L = ops.L
    d, x, dy = _wgrad_operands(ops, dev)
    xd, dyd = x.to(dev), dy.to(dev)
    nb = L.lib.rh_conv1d_workspace_bytes(C.byref(d))
    st = L.stream()
    rx, rdy = _amax_slot(ops, xd), _amax_slot(ops, dyd)
    # the shape is K-split: armed and valid, the call leaves its partials to the caller
    probe = L.ReduceItem()
    ws0 = _ws(ops, nb, dev)
    dw0 = torch.empty(96, 96, 3, device=dev)
    L.lib.rh_x6_set_ranges(L.ptr(rdy), L.ptr(rx), None, None)
    L.lib.rh_defer_reduce(C.byref(probe))
    L.check(L.lib.rh_conv1d_bwd_weight_f32(C.byref(d), L.ptr(dyd), L.ptr(xd), None, L.ptr(dw0), None, L.ptr(ws0), nb, st), "probe")
    assert probe.Z > 1
    L.check(L.lib.rh_reduce_partials_batched_f32(C.byref(probe), 1, st), "reduce")
    # armed, then a failing call
    item = L.ReduceItem()
    L.lib.rh_defer_reduce(C.byref(item))
    assert L.lib.rh_conv1d_bwd_weight_f32(C.byref(d), L.ptr(dyd), L.ptr(xd), None, None, None, None, 0, st) == -1
    # the next valid weight gradient (slots armed, no defer): reduced by the call itself
    ws = _ws(ops, nb, dev)
    dw = torch.full((96, 96, 3), float("nan"), device=dev)
    L.lib.rh_x6_set_ranges(L.ptr(rdy), L.ptr(rx), None, None)
    L.check(L.lib.rh_conv1d_bwd_weight_f32(C.byref(d), L.ptr(dyd), L.ptr(xd), None, L.ptr(dw), None, L.ptr(ws), nb, st), "wgrad")
    torch.cuda.synchronize()
    assert (item.part, item.out, item.n, item.Z) == (None, None, 0, 0)
    dw64 = torch.nn.grad.conv1d_weight(x.double(), (96, 96, 3), dy.double(), padding=1)
    assert torch.isfinite(dw).all()
    assert rel_l2(dw.cpu().double(), dw64) < 2e-6
    assert torch.equal(dw, dw0)


def test_armed_kernel_events_are_dropped_by_a_failing_call(f16, dev):
    """rh_set_kernel_events then a failing call: the events must not ride on the next call's main kernel."""
    ops = f16
    L = ops.L
    d3, d1 = _unit_descs(ops)
    h0, h1 = C.c_void_p(), C.c_void_p()
    L.check(L.lib.rh_event_create(C.byref(h0)), "ev")
    L.check(L.lib.rh_event_create(C.byref(h1)), "ev")
    try:
        L.lib.rh_set_kernel_events(h0, h1)
        assert L.lib.rh_conv1d_fwd_f32(C.byref(d3), None, None, None, None, None, None, None, 0, L.stream()) == -1
        gen = torch.Generator().manual_seed(73)
        xd = torch.randn(2, 96, 256, generator=gen).to(dev)
        wp, _, _ = ops._pack(d3, (torch.randn(96, 96, 3, generator=gen) / 17).to(dev), None, False, dev, L.stream())
        y = torch.empty_like(xd)
        rin, rout = _amax_slot(ops, xd), _zslot(ops, dev)
        L.lib.rh_x6_set_ranges(None, L.ptr(rin), L.ptr(rout), None)
        L.check(L.lib.rh_conv1d_fwd_f32(C.byref(d3), L.ptr(xd), L.ptr(wp), None, None, None, L.ptr(y), None, 0, L.stream()), "conv")
        assert L.lib.rh_kernel_events_used() == 0
        torch.cuda.synchronize()
    finally:
        L.lib.rh_kernel_events_used()
        L.lib.rh_event_destroy(h0)
        L.lib.rh_event_destroy(h1)
