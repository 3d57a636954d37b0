"""Host-only proof that tests/x6_matrix.py covers conv_x6_kernel: every row plans to exactly the instance it names (a change
that re-routes a geometry fails here and must update the table), and the coverage conditions hold over those keys.  No GPU:
rh_conv1d_plan_info is a pure function of the descriptor.  tests/test_gpu_x6_matrix.py runs the same rows on the GPU."""
import ctypes as C
import os

import pytest

import x6_matrix as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = os.path.join(ROOT, "profiles", "conv_x6_instance_matrix.txt")
X6_ROWS = [r for r in X.ROWS if r.key is not None]
ALL_SHAPES = [(IS,) + s for IS in (1, 2, 4) for s in X.SHAPES]
# operand modes the C ABI can express: forward = bias / add / output LeakyReLU with either input; data gradient = derivative / add
FWD_MODES = [(lk, m) for lk in (False, True) for m in (0, 1, 4, 5, 9, 13) if X.epi_instantiated(1, 3, lk, m)]
DGRAD_MODES = [(False, m) for m in (0, 2, 4, 6)]
OPS_OF = {0: "", 1: "b", 4: "a", 5: "ba", 9: "bo", 13: "bao"}
EDGES = ["ragged last column tile", "nb > 1", "B % nb != 0", "ncols == 1", "ncols == bnl - 1", "ncols == bnl + 1", "M < Mp",
         "partial last row tile at wm == 2", "causal padding", "padding beyond the left halo", "largest staged row that fits LDS"]


@pytest.fixture(scope="module")
def L():
    from rave_amd import _lib
    X.assert_default_planner_env()
    return _lib


def _group(key):
    """Edges are asked for each IS, and for each tn at IS == 1."""
    return (1, key.tn) if key.IS == 1 else (key.IS, 0)


@pytest.mark.parametrize("row", X.ROWS, ids=[r.name for r in X.ROWS])
def test_row_plans_to_its_key(L, row):
    assert X.derive_key(L, row) == row.key, (row.name, X.fmt_key(X.derive_key(L, row)), X.fmt_key(row.key))


def test_shapes_and_k_modes():
    keys = [r.key for r in X6_ROWS]
    for sh in ALL_SHAPES:
        for km in ("unsplit", "combine"):
            assert any((k.IS, k.tm, k.tn, k.wm) == sh and k.kmode == km for k in keys), (sh, km)
    # all four K modes for each IS, and for each tm at IS == 1
    for km in X.KMODES:
        for tm in (1, 2, 3):
            assert any(k.IS == 1 and k.tm == tm and k.kmode == km for k in keys), (1, tm, km)
        for IS in (2, 4):
            assert any(k.IS == IS and k.kmode == km for k in keys), (IS, km)
    # the finalize pass applies the operands the kernel's epilogue otherwise does: each of them
    for bit, what in ((1, "bias"), (4, "add"), (2, "derivative")):
        assert any(k.kmode == "finalize" and k.epi & bit for k in keys), what
    assert any(k.multiphase and k.kmode == "unsplit" for k in keys) and any(k.multiphase and k.kmode != "unsplit" for k in keys)


def test_operand_modes():
    ran = {(k.IS, k.vs, k.leaky, k.epi) for k in (r.key for r in X6_ROWS) if k.kmode != "finalize"}
    for IS in (1, 2, 4):
        for lk, m in FWD_MODES + DGRAD_MODES:
            assert (IS, 0, lk, m) in ran, (IS, lk, m)
    for vs in (2, 4):
        for lk in (False, True):
            for m in range(16):
                if X.epi_instantiated(1, 2, lk, m | 16):
                    assert (1, vs, lk, m) in ran, (vs, lk, m)
    # every listed mode is an instance, and every instantiated mode is listed: the ABI reaches all of rh_x6_epi_instantiated
    assert {(lk, m) for lk, m in FWD_MODES + DGRAD_MODES} == {(lk, m) for lk in (False, True) for m in range(16)
                                                                 if X.epi_instantiated(1, 3, lk, m)}


def test_edges(L):
    have = {}
    for r in X6_ROWS:
        have.setdefault(_group(r.key), set()).update(X.edges(r, X.plan_info(L, r)))
    for grp in ((1, 1), (1, 2), (2, 0), (4, 0)):
        for e in EDGES:
            if grp == (4, 0) and e == "largest staged row that fits LDS":
                # IS == 4: the staged row is bnl + ceil(k / 4) - 1 <= bnl + 15 positions (k <= 64 taps) and the tightest tile
                # (tn = 2, wm = 1: nb = 8 items of bnl = 32) fits 32 + 16: the bound cannot be reached
                continue
            assert e in have[grp], (grp, e)
    # the smallest staged rows that no longer fit: the sibling of a row on the bound plans to tn = 1 or to the f32 kernels
    over = [r for r in X.ROWS if r.key is None]
    assert len(over) >= 2 and all(X.plan_info(L, r)[0] == 0 for r in over)
    sib = {r.geo: r for r in X.ROWS}
    a, b = sib[(1, 16, 128, 49157, 3, 1, 64, (64, 64), False)], sib[(1, 16, 128, 49157, 3, 1, 65, (64, 64), False)]
    assert (a.key.tn, b.key.tn) == (2, 1) and "largest staged row that fits LDS" in X.edges(a, X.plan_info(L, a))


def test_batch_folding_is_real_for_each_staging_and_epilogue(L):
    """The IS > 1 staging and the virtual-row epilogue address the folded batch items in code of their own: each of them, forward
    and data gradient, has a row with B > nb > 1 and B % nb != 0, and one of those split in K."""
    folded = [r for r in X6_ROWS if "B % nb != 0" in X.edges(r, X.plan_info(L, r))]
    for which in (0, 1):
        for IS in (2, 4):
            assert any(r.key.which == which and r.key.IS == IS for r in folded), (which, IS)
            assert any(r.key.IS == IS and r.key.kmode in ("combine", "finalize") for r in folded), IS
        for vs in (2, 4):
            assert any(r.key.which == which and r.key.vs == vs for r in folded), (which, vs)
            assert any(r.key.vs == vs and r.key.kmode in ("combine", "finalize") for r in folded), vs


def test_every_shape_runs_the_plain_and_derivative_modes():
    """The thinning: shapes exhaustively on the kernel's modes 0 and 5 (plain input) and on the derivative mode 2."""
    ran = {(k.IS, k.tm, k.tn, k.wm, k.leaky, X.kernel_epi(k) & 15) for k in (r.key for r in X6_ROWS)}
    for sh in ALL_SHAPES:
        for m in (0, 5, 2):
            assert sh + (False, m) in ran, (sh, m)


def _mirror(r):
    """The call of the OTHER entry point with the same GEMM (rows, K, columns, taps): the data gradient of a transposed conv
    gathers like the forward of a strided one and so on (conv_host.hip: build_plan).  None = no such call."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = r.geo
    span = (k - 1) * dil
    if r.which == 0 and not tr:
        n = X.out_len(r.geo)
        geo = (B, Co, Ci, n, k, s, 1, (pad[0], 0), True) if s > 1 else (B, Co, Ci, n, k, 1, dil, (span // 2, span - span // 2), False)
    elif r.which == 0:
        geo = (B, Co, Ci, X.out_len(r.geo), k, s, 1, (pad[0], max(0, k - s - pad[0])), False)
    elif tr:
        geo = (B, Co, Ci, (Lx - 1) * s + k - pad[0], k, s, 1, (pad[0], 0), False)
    elif s == 1:
        geo = (B, Co, Ci, Lx, k, 1, dil, (span // 2, span - span // 2), False)
    else:
        fit = [n for n in range(1, Lx + 2) if -(-((n - 1) * s - 2 * pad[0] + k) // s) == -(-Lx // s)]
        if not fit:
            return None
        geo = (B, Co, Ci, fit[0], k, s, 1, (pad[0], pad[0]), True)
    if geo[3] < 1 or X.out_len(geo) < 1:
        return None
    return r._replace(which=1 - r.which, geo=geo, ops="")


def _reach(L, want):
    """True if some table row of the instance's tile shape (or its mirror), with its operand flags swapped, plans to ``want``."""
    IS, tm, tn, wm, leaky, epi = want
    vs, m = {0: 0, 1: 2, 2: 4}[epi >> 4], epi & 15
    same = [r for r in X6_ROWS if (r.key.IS, r.key.tm, r.key.tn, r.key.wm, r.key.vs) == (IS, tm, tn, wm, vs)]
    for r in same + [q for q in map(_mirror, same) if q is not None]:
        k = r
        if k.which == 0 and m in OPS_OF:
            ops = ("L" if leaky else "") + OPS_OF[m]
        elif k.which == 1 and not leaky and m in (0, 2, 4, 6):
            ops = ("L" if m & 2 else "") + ("a" if m & 4 else "")
        else:
            continue
        k2 = X.derive_key(L, r._replace(ops=ops))
        if k2 is not None and (k2.IS, k2.tm, k2.tn, k2.wm, k2.leaky, X.kernel_epi(k2)) == want:
            return True
    return False


def test_every_instantiated_pair_is_reachable_or_listed(L):
    inst = X.instances()
    assert len(inst) == 30 * 12 + 8 * 18
    listed = {u[0] for u in X.UNREACHABLE}
    assert all(u in inst for u in listed) and all(isinstance(u[1], str) and u[1] for u in X.UNREACHABLE)
    assert len(listed) <= 0.05 * len(inst)
    for sh in ALL_SHAPES:
        assert any(i[:4] == sh and i not in listed for i in inst), sh
    unproven = [i for i in inst if i not in listed and not _reach(L, i)]
    assert not unproven, unproven
    # the launcher's list (x6_launch: RH_X6_E) against the planner's (rh_x6_epi_instantiated) is checked by the GPU test: a mode
    # the planner accepts and the launcher lacks fails the launch with RH_ERR_UNSUPPORTED


def test_operand_sets_without_an_instance_plan_to_the_f32_kernels(L):
    base = dict(batch=3, c_in=96, c_out=96, l_in=257, l_out=257, kernel=3, stride=1, dilation=9, pad_left=9, transposed=0, groups=1,
                inner=1, in_valid=0, act=1, act_slope=0.2, out_act=0, out_slope=0.1)

    def fam(which, has_bias=0, has_add=0, **kw):
        out = (C.c_int32 * 8)()
        L.check(L.lib.rh_conv1d_plan_info(C.byref(L.ConvDesc(**dict(base, **kw))), which, has_bias, has_add, out), "plan_info")
        return out[0]

    assert fam(0) == 1 and fam(1) == 1 and fam(0, 1, 1, act=0, out_act=1) == 1
    assert fam(0, 0, 0, act=0, out_act=1) == 0 and fam(0, 0, 1, act=0, out_act=1) == 0   # output LeakyReLU without bias
    assert fam(0, 1, 0, out_act=1) == 0                                          # ... or behind a LeakyReLU input
    assert fam(0, act=2) == 0 and fam(1, act=2) == 0                             # snake: input activation / derivative
    assert fam(0, act_slope=1.5) == 0 and fam(0, act_slope=-0.1) == 0            # applied as max(x, slope x)
    assert fam(1, act_slope=1.5) == 1                                            # the derivative takes any slope
    # (derivative with a LeakyReLU input: no call can ask for it, x6_matrix.INEXPRESSIBLE)


def _ledger(L):
    lines = ["conv_x6_kernel instance matrix (tests/x6_matrix.py; written by tests/test_x6_matrix_host.py)", ""]
    for r in X.ROWS:
        e = sorted(X.edges(r, X.plan_info(L, r))) if r.key is not None else []
        lines.append(f"{r.name:58s} | {X.fmt_key(r.key)}" + (f" | {', '.join(e)}" if e else ""))
    keys = {(k.IS, k.tm, k.tn, k.wm, k.leaky, k.epi | {0: 0, 2: 16, 4: 32}[k.vs], k.kmode) for k in (r.key for r in X6_ROWS)}
    pairs = {(k.IS, k.tm, k.tn, k.wm, k.leaky, X.kernel_epi(k)) for k in (r.key for r in X6_ROWS)}
    # reachable keys: the tile shape and the K split follow the sizes, the mode the operands, the K mode the slices / workspace /
    # RH_X6_COMBINE -- independently, so every reachable pair is reachable in each of the four K modes
    reachable = 4 * (len(X.instances()) - len(X.UNREACHABLE))
    lines += ["", f"{len(X.ROWS)} rows; {len(keys)} of the {reachable} reachable (shape, operand mode, K mode) keys; {len(pairs)} of the "
                  f"{len(X.instances())} instantiated (shape, mode) kernel instances run, every one proven reachable on the host",
              "unreachable instances: " + ("none" if not X.UNREACHABLE else "")]
    lines += [f"  {u[0]}: {u[1]}" for u in X.UNREACHABLE]
    lines += ["not expressible through the C ABI: " + "; ".join(X.INEXPRESSIBLE)]
    return "\n".join(lines) + "\n"


def test_ledger_is_current(L):
    """The committed ledger is what the table and the planner give today (this test writes nothing)."""
    assert os.path.exists(LEDGER) and open(LEDGER).read() == _ledger(L), \
        "profiles/conv_x6_instance_matrix.txt is stale: write it again with `python tests/test_x6_matrix_host.py`"


if __name__ == "__main__":     # writes the ledger
    import sys
    sys.path.insert(0, ROOT)
    from rave_amd import _lib
    X.assert_default_planner_env()
    with open(LEDGER, "w") as f:
        f.write(_ledger(_lib))
