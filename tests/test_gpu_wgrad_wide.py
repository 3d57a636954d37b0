"""The column-complete weight-gradient tile (rave_amd/csrc/conv_wgrad_x6.hip: wgrad_x6_wide_kernel) for layers with 65 ... 96
gradient rows and at most 288 columns: one workgroup tile over the whole weight tensor, one wave per 32 columns.

A per-output-element sum depends only on the K slicing, the step order and the product order, not on which wave owns the
column.  So with the K slicing of the 4-wave plan (``RH_WGRAD_X6_WIDE=2``) the wide tile must give the SAME BITS as the 4-wave path
(``RH_WGRAD_X6_WIDE=0``), for the weight and the bias gradient; with its own slicing it stays within 2e-6 (relative L2) of the
exact-f32 MFMA kernels (``RH_WGRAD_X6=0``) and two runs of one call give the same bits.  Which kernel and which slicing a call
takes is read from the library (``rh_conv1d_bwd_weight_plan_info``), so that none of this compares the 4-wave path with itself.

These are the workload's shapes through autograd, compared among the project's own kernels.  Every instance of both kernels
against an independent f64 reference, slice by slice and at the tile edges, is tests/test_gpu_wgrad_matrix.py (table:
tests/wgrad_matrix.py, coverage proof: tests/test_wgrad_matrix_host.py).
"""
import importlib.util
import os
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def rel_l2(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


class _Env:
    """Sets the given variables; a value of None removes the variable for the duration."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# the switches a wide-tile run must not inherit from the caller's environment
CLEAN = dict(RH_WGRAD_X6=None, RH_WGRAD_X6_PLANES=None, RH_WGRAD_X6_BLOCKS=None, RH_WGRAD_X6_WIDE=None)

WIDE_CASES = [
    # (name, batch, c_in, c_out, length, kernel, geometry kwargs, waves)          N = c_in * kernel columns, M = c_out rows
    ("unit_k3_d1_c96", 8, 96, 96, 4096, 3, dict(dilation=1, pad_left=1, pad_right=1, act=1, slope=0.2), 9),
    ("unit_k3_d9_c96", 8, 96, 96, 4096, 3, dict(dilation=9, pad_left=9, pad_right=9, act=1, slope=0.2), 9),
    ("unit_k3_d1_c96_causal_ragged", 3, 96, 96, 4001, 3, dict(dilation=1, pad_left=2, pad_right=0, act=1, slope=0.2), 9),
    ("unit_k3_d9_c96_causal_ragged", 3, 96, 96, 4001, 3, dict(dilation=9, pad_left=18, pad_right=0, act=1, slope=0.2), 9),
    ("unit_k1_c96", 8, 96, 96, 4096, 1, dict(act=1, slope=0.2), 3),
    ("stem_16_96_k7", 8, 16, 96, 4096, 7, dict(pad_left=3, pad_right=3), 4),
    ("ragged_m80_n75_k3", 5, 25, 80, 1003, 3, dict(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2), 3),
    ("ragged_m70_n170_k1", 4, 170, 70, 2050, 1, dict(act=1, slope=0.2), 6),
    ("strided_k4s2_60_96", 4, 60, 96, 2048, 4, dict(stride=2, pad_left=1, pad_right=1, act=1, slope=0.2), 9),
    # nine waves over ONE 4-wave column tile (N = 240 <= 256), long enough that the "at least four steps per slice" clamp does not
    # decide: the 4-wave plan takes 512 slices, the wide plan's own choice is 256
    ("unit_k3_d3_c80_long", 16, 80, 96, 4096, 3, dict(dilation=3, pad_left=3, pad_right=3, act=1, slope=0.2), 9),
]
# the 32-row output layer (672 columns) stays on the f32-input MFMA kernel under every switch
OUT_LAYER = ("out_96_32_k7", 8, 96, 32, 4096, 7, dict(pad_left=3, pad_right=3, act=1, slope=0.2), 0)


def _plan(case, **env):
    """{waves per workgroup, workgroups, K slices, planes} of the weight-gradient launch the library would issue for the case."""
    import ctypes as C
    from rave_amd import _lib as L
    from rave_amd.ops import ConvGeom, _desc
    _, batch, c_in, c_out, length, k, kw, _ = case
    geom = ConvGeom(**kw)
    d = _desc(geom, batch, c_in, c_out, length, geom.out_len(length, k), k)
    out = (C.c_int32 * 4)()
    with _Env(**{**CLEAN, **env}):
        L.check(L.lib.rh_conv1d_bwd_weight_plan_info(C.byref(d), out), "plan_info")
        ws = L.lib.rh_conv1d_workspace_bytes(C.byref(d))
    return dict(waves=out[0], workgroups=out[1], slices=out[2], planes=out[3], ws=ws)


def _runner(dev, case):
    from rave_amd import ops as R
    from rave_amd.ops import ConvGeom
    _, batch, c_in, c_out, length, k, kw, _ = case
    gen = torch.Generator().manual_seed(41)
    geom = ConvGeom(**kw)
    x = torch.randn(batch, c_in, length, generator=gen).to(dev)
    w0 = (torch.randn(c_out, c_in, k, generator=gen) * 0.05).to(dev)
    b0 = torch.randn(c_out, generator=gen).to(dev)

    def run(**env):
        with _Env(**{**CLEAN, "RH_BWD_SIDE_STREAM": 0, **env}):
            w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            y = R.conv1d(x, w, b, geom=geom)
            cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(42)).to(dev)
            y.backward(cot)
            torch.cuda.synchronize()
            return w.grad.clone(), b.grad.clone()
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_wide_tile_with_the_four_wave_slicing_is_bit_identical(dev, case):
    four, same = _plan(case, RH_WGRAD_X6_WIDE=0), _plan(case, RH_WGRAD_X6_WIDE=2)
    assert four["waves"] == 4 and same["waves"] == case[7]                  # the two runs below really are the two kernels
    assert same["slices"] == four["slices"] and same["ws"] == four["ws"]
    run = _runner(dev, case)
    dw4, db4 = run(RH_WGRAD_X6_WIDE=0)
    assert torch.isfinite(dw4).all()
    dwf, dbf = run(RH_WGRAD_X6=0)
    dww, dbw = run(RH_WGRAD_X6_WIDE=2)
    assert torch.equal(dww, dw4), rel_l2(dww, dw4)
    assert torch.equal(dbw, db4), rel_l2(dbw, db4)
    ew, eb = rel_l2(dww, dwf), rel_l2(dbw, dbf)
    print(f"{case[0]}: rel L2 against the f32 kernels: dw {ew:.3e} db {eb:.3e}")
    assert ew < 2e-6 and eb < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_wide_tile_with_its_own_slicing_is_exact_and_deterministic(dev, case):
    run = _runner(dev, case)
    dwf, dbf = run(RH_WGRAD_X6=0)
    for env in (dict(), dict(RH_WGRAD_X6_BLOCKS=1000)):
        assert _plan(case, **env)["waves"] == case[7]
        dw1, db1 = run(**env)
        dw2, db2 = run(**env)
        assert torch.isfinite(dw1).all()
        assert torch.equal(dw1, dw2) and torch.equal(db1, db2), env
        ew, eb = rel_l2(dw1, dwf), rel_l2(db1, dbf)
        print(f"{case[0]} {env}: rel L2 against the f32 kernels: dw {ew:.3e} db {eb:.3e}")
        assert ew < 2e-6 and eb < 2e-6, env


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES + [OUT_LAYER], ids=[c[0] for c in WIDE_CASES + [OUT_LAYER]])
def test_the_plan_takes_the_wide_tile_exactly_where_it_says(dev, case):
    """By default a layer with 65 ... 96 rows and <= 288 columns takes the wide tile with one wave per 32 columns (rounded up to
    3, 4, 6, 9) and one workgroup per K slice; RH_WGRAD_X6_WIDE=0 and a forced RH_WGRAD_X6_PLANES select the 4-wave kernel, and
    RH_WGRAD_X6_WIDE=2 the wide tile with the 4-wave plan's slices.  The scratch the library asks for (Z x (M x N + M) floats of
    partials) answers for the plan the launch will take.  The 32-row output layer is left alone by every switch."""
    name, batch, c_in, c_out, length, k, kw, waves = case
    own, four, same = _plan(case), _plan(case, RH_WGRAD_X6_WIDE=0), _plan(case, RH_WGRAD_X6_WIDE=2)
    if waves == 0:
        for pl in (own, four, same, _plan(case, RH_WGRAD_X6_PLANES=1)):
            assert pl["waves"] == 0 and pl["ws"] == own["ws"]
        return
    n = c_in * k
    assert 32 * waves >= n and own["waves"] == waves and own["workgroups"] == own["slices"]
    assert own["planes"] == int(k > 1 and kw.get("stride", 1) == 1)
    assert four["waves"] == 4 and four["workgroups"] == four["slices"] * -(-n // 256)
    assert same["waves"] == waves and same["slices"] == four["slices"] and same["ws"] == four["ws"]
    for planes in (0, 1):
        forced = _plan(case, RH_WGRAD_X6_PLANES=planes)
        assert forced["waves"] == 4 and forced["slices"] == four["slices"] and forced["ws"] == four["ws"]
    # 64 workgroups asked for: one column tile -> up to 64 slices; the 4-wave plan of a two-tile layer (N > 256) takes 32
    wide64, four64 = _plan(case, RH_WGRAD_X6_BLOCKS=64), _plan(case, RH_WGRAD_X6_WIDE=0, RH_WGRAD_X6_BLOCKS=64)
    assert wide64["workgroups"] == wide64["slices"] <= 64
    if n > 256:
        assert wide64["slices"] > four64["slices"] and wide64["ws"] > four64["ws"]
    else:
        assert wide64["slices"] == four64["slices"] and wide64["ws"] == four64["ws"]
    if name == "unit_k3_d3_c80_long":       # own slicing: one resident round of nine-wave workgroups; the 4-wave plan: 512
        assert (own["slices"], four["slices"]) == (256, 512)


def test_wide_tile_instances_use_no_scratch():
    """The accumulators (48 registers per wave) and the staged samples stay in registers: no private segment, no spills, read
    back from the built library like tests/test_abi_and_host.py does for the other MFMA kernels; and the nine-wave instances
    fit the 168 registers that three waves per SIMD leave (a 576-thread workgroup needs three wave slots on one SIMD)."""
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    wide = [k for k in kr.kernels() if "wgrad_x6_wide_kernel" in k["name"]]
    assert len(wide) == 8, [k["name"] for k in wide]              # 3, 4, 6, 9 waves x {per-column, plane} staging
    bad = [k for k in wide if k["scratch"] or k["vgpr_spill"]]
    assert not bad, bad
    assert not [k for k in kr.scratch_kernels() if "wide" in k["name"]]       # and the tool's own list knows the new name
    for k in wide:
        if "ILi9E" in k["name"]:
            assert k["vgpr"] + k["agpr"] <= 168, k
