"""Host-only proof that tests/f32_matrix.py covers the f32-input MFMA forward / data-gradient kernels: every row plans to exactly the
instance it names (a change that re-routes a geometry fails here and must update the table), and the coverage conditions hold over
the rows.  No GPU: rh_conv1d_f32_instance_info is a pure function of the descriptor and the flags, answered by the planning code
the launch itself runs.  tests/test_gpu_f32_matrix.py runs the same rows on the GPU."""
import ctypes as C
import os

import pytest

import f32_matrix as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = os.path.join(ROOT, "profiles", "conv_f32_instance_matrix.txt")


@pytest.fixture(scope="module")
def L():
    from rave_amd import _lib
    X.assert_default_planner_env()
    return _lib


@pytest.fixture(scope="module")
def tags(L):
    return {r.name: X.tags_of(L, r) for r in X.ROWS}


def _all(tags):
    return set().union(*tags.values())


@pytest.mark.parametrize("row", X.ROWS, ids=[r.name for r in X.ROWS])
def test_row_plans_to_its_key(L, row):
    assert row.key is not None and X.derive_key(L, row) == row.key, (row.name, X.fmt_key(X.derive_key(L, row)), X.fmt_key(row.key))


def test_rows_are_small():
    """Tens to a few hundred positions, batch <= 5, channels <= 200; the long staged rows have B = 1 and 2 - 4 input channels."""
    for r in X.ROWS:
        B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = r.geo
        assert B <= 5 and max(Ci, Co) <= 200, r.name
        assert Lx * inner <= 400 or (B == 1 and 2 <= X.gemm(r)["C"] <= 4 and Lx <= 12000), r.name


def test_every_instance_is_hit(tags):
    have = _all(tags)
    assert len(X.dma_instances()) == 24 and len(X.UNREACHABLE) <= 2
    listed = {u[0] for u in X.UNREACHABLE}
    for s, lk, v in X.dma_instances():
        assert ("dma", s, lk, v) in have or ("dma", s, lk, v) in listed, (s, lk, v)
    for s in X.SHAPES:
        assert ("sync", s) in have and ("sync by a Snake forward", s) in have, s
    assert ("sync by the LDS fallback",) in have
    # the key never names the pair launch_dma does not instantiate
    assert all(r.key.vec or r.key.ctail for r in X.ROWS if r.key.kernel == 1)


def test_k_modes(tags):
    have = _all(tags)
    for s in X.SHAPES:
        for km in X.KMODES:
            assert ("kmode", s, km) in have, (s, km)
    for f in (1, 4):
        for o in X.FINALIZE_OPERANDS:
            assert ("finalize", f, o) in have, (f, o)


def test_phases_and_inner(tags):
    have = _all(tags)
    for n in (2, 3, 4):
        for m in ("unsplit", "split"):
            assert ("phases", n, m) in have, (n, m)
    assert ("inner", 0) in have and ("inner", 1) in have and ("inner, nb > 1",) in have


def test_edges_per_tile_shape(L, tags):
    have = _all(tags)
    for s in X.SHAPES:
        for e in X.EDGES:
            assert ("edge", s, e) in have, (s, e)
    # the siblings: the row on a bound and the first staged row beyond it differ by one dilation step of at most 4 positions
    def pair(s, a_edge, b_edge):
        on = [r for r in X.ROWS if ("edge", s, a_edge) in tags[r.name]]
        off = [r for r in X.ROWS if ("edge", s, b_edge) in tags[r.name]]
        return any(a.geo[:3] == b.geo[:3] and a.geo[4:6] == b.geo[4:6] and 0 < b.geo[6] - a.geo[6] <= 64 and b.geo[3] - a.geo[3] == b.geo[6] - a.geo[6]
                   for a in on for b in off)
    for s in X.SHAPES:
        assert pair(s, "last staged row that fits nx <= 8", "VEC refused for its DMA slots"), s
        assert pair(s, "last geometry within 160 KiB of LDS", "DMA stages beyond 160 KiB of LDS: synchronous kernel"), s


def test_dead_conditions(L):
    """maxtaps > 64 switches VEC off in plan_dma; no descriptor gets there."""
    d = L.ConvDesc(batch=1, c_in=4, c_out=4, l_in=200, l_out=136, kernel=65, stride=1, dilation=1, pad_left=0, transposed=0, groups=1,
                   inner=1, in_valid=0, act=0, act_slope=0.0, out_act=0, out_slope=0.0)
    out = (C.c_int32 * 24)()
    assert L.lib.rh_conv1d_f32_instance_info(C.byref(d), 0, 0, 0, 1, 1, out) != 0 and b"kernel" in L.lib.rh_last_error()
    assert len(X.DEAD_CONDITIONS) == 1


def magic_of(d):
    return ((1 << 20) + d - 1) // d                      # conv_igemm_dma.hip: magic_of


def mdiv20(n, magic):
    return ((n * magic) & 0xFFFFFFFF) >> 20              # conv_igemm_dma.hip: mdiv20 (32-bit product)


def reciprocal_failures():
    """Every (divisor, n) an accepted plan of plan_dma can hand to mdiv20 (bounds from plan_dma and the kernel's loops, NW = 4 waves):
    magic_lpr -- VEC only: slot g < 8 * 64 * NW = 2048 by lpr <= 2048 / xrows (nx <= 8), xrows = nb * ck even and >= 2; the quotient
                 must be exact for g < xrows * lpr and at least xrows beyond (those slots are switched off by row < xrows);
    magic_ck  -- row < xrows <= 8 * 32 of the staged input, and weight row kr < 64 taps * 32 channels + one DMA instruction, by ck <= 32;
    magic_segs -- computed by plan_dma, read by no kernel.
    Returns the failing (what, d, n) with and without the planner's refusal of VEC beyond (xrows * lpr - 1) * lpr < 2^20."""
    bad, bad_refused = [], []
    for xrows in range(2, 257, 2):
        for lpr in range(1, 2048 // xrows + 1):
            m = magic_of(lpr)
            ok = all(mdiv20(g, m) == g // lpr for g in range(xrows * lpr)) and all(mdiv20(g, m) >= xrows for g in range(xrows * lpr, 2048))
            if not ok:
                bad.append(("lpr", xrows, lpr))
                if (xrows * lpr - 1) * lpr < 1 << 20:
                    bad_refused.append(("lpr", xrows, lpr))
    for ck in range(2, 33, 2):
        m = magic_of(ck)
        if any(mdiv20(n, m) != n // ck for n in range(64 * 32 + 256)):
            bad.append(("ck", ck))
            bad_refused.append(("ck", ck))
    return bad, bad_refused


def test_20_bit_reciprocals(L, tags):
    bad, bad_refused = reciprocal_failures()
    # without the refusal the slot division fails exactly for two staged rows of 724 .. 1024 float4 each (the smallest: 756)
    assert bad and all(b[0] == "lpr" and b[1] == 2 and 724 <= b[2] <= 1024 for b in bad) and min(b[2] for b in bad) == 756, bad[:5]
    assert (magic_of(756), mdiv20(1511, magic_of(756)), 1511 // 756) == (1388, 2, 1)      # the last float4 of the second row
    assert not bad_refused, bad_refused
    # the planner does refuse: the smallest failing geometry is in the table and plans to the element-wise variant
    rows = [r for r in X.ROWS if ("staged row beyond the exact range of the 20-bit reciprocal",) in tags[r.name]]
    assert rows and all(not r.key.vec for r in rows)
    assert any(X.vec_plan0(r, X.instance_info(L, r)) == (2, 756) for r in rows)


def test_some_twin_is_compared_bit_for_bit(L):
    """Check d of the GPU test must not be vacuous: VEC rows whose 4-byte-aligned twin plans to the same ck and K slices exist."""
    n = 0
    for row in X.ROWS:
        if row.key.vec:
            a, b = X.instance_info(L, row), X.instance_info(L, row, align=4)
            n += (a.ck, a.ks) == (b.ck, b.ks)
    assert n >= 4, n


def _ledger(L):
    lines = ["f32-input MFMA forward / data-gradient instance matrix (tests/f32_matrix.py; written by tests/test_f32_matrix_host.py)", ""]
    for r in X.ROWS:
        e = sorted(X.edges(r, X.instance_info(L, r)))
        lines.append(f"{r.name:62s} | {X.fmt_key(r.key)}" + (f" | {', '.join(e)}" if e else ""))
    dma = {(k.TM, k.TN, k.WM, k.WN, k.leaky, k.vec, k.ctail) for k in (r.key for r in X.ROWS) if k.kernel == 1}
    sync = {(k.TM, k.TN, k.WM, k.WN) for k in (r.key for r in X.ROWS) if k.kernel == 0}
    keys = {r.key for r in X.ROWS}
    # reachable keys: instance x the four K modes for the DMA kernel (the tile shape follows M, the variant the alignment and C, the K
    # mode the slices / workspace), the synchronous kernel runs unsplit only; each x which x phases x inner is not counted
    reachable = 4 * (24 - len(X.UNREACHABLE)) + 4
    lines += ["", f"{len(X.ROWS)} rows; {len(dma)} of the 24 instantiated conv_igemm_dma_kernel instances and {len(sync)} of the 4 "
                  f"conv_igemm_kernel instances run; {len({(k.kernel, k.TM, k.TN, k.WM, k.WN, k.leaky, k.vec, k.ctail, k.kmode) for k in keys})} of the "
                  f"{reachable} reachable (instance, K mode) keys; {len(keys)} distinct keys in all",
              "unreachable instances: " + ("none" if not X.UNREACHABLE else "")]
    lines += [f"  {u[0]}: {u[1]}" for u in X.UNREACHABLE]
    lines += ["conditions of the code no call can reach: " + "; ".join(X.DEAD_CONDITIONS)]
    return "\n".join(lines) + "\n"


def test_ledger_is_current(L):
    """The committed ledger is what the table and the planner give today (this test writes nothing)."""
    assert os.path.exists(LEDGER) and open(LEDGER).read() == _ledger(L), \
        "profiles/conv_f32_instance_matrix.txt is stale: write it again with `python tests/test_f32_matrix_host.py`"


if __name__ == "__main__":     # writes the ledger
    import sys
    sys.path.insert(0, ROOT)
    from rave_amd import _lib
    X.assert_default_planner_env()
    with open(LEDGER, "w") as f:
        f.write(_ledger(_lib))
