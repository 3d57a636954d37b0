"""Host-only proof that tests/wgrad_matrix.py covers the 1-D weight-gradient kernels: every row launches exactly the instance it
names (a change that re-routes a geometry fails here and must update the table), every one of the 48 x6 instances and every
reachable f32-input instance has a row, and every listed edge occurs for every kernel kind it exists for.  No GPU:
rh_conv1d_bwd_weight_instance_info is a pure function of the descriptor, the alignment flags and the per-call switches, answered
by route_wgrad1 (csrc/conv_wgrad.hip), the function the launch itself goes through; the scratch query is a caller of it too.
tests/test_gpu_wgrad_matrix.py runs the same rows on the GPU."""
import ctypes as C
import os

import pytest

import wgrad_matrix as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = os.path.join(ROOT, "profiles", "wgrad_instance_matrix.txt")


@pytest.fixture(scope="module")
def L():
    from rave_amd import _lib
    W.assert_default_planner_env()
    return _lib


@pytest.mark.parametrize("row", W.ROWS, ids=[r.name for r in W.ROWS])
def test_row_launches_its_key(L, row):
    info = W.instance_info(L, row)
    assert W.key_of(info) == row.key, (row.name, W.fmt_key(W.key_of(info)), W.fmt_key(row.key))
    # the older diagnostic agrees where it answers at all: {waves, workgroups, K slices, planes}
    out = (C.c_int32 * 4)()
    with W.call_env(row):
        L.check(L.lib.rh_conv1d_bwd_weight_plan_info(C.byref(W.desc(L, row)), out), "plan_info")
    if info[0] == 1:
        assert tuple(out) == (info[2] if info[1] else 4, info[15] * info[7], info[7], info[6]), (tuple(out), info)


def test_rows_are_small():
    for r in W.ROWS:
        B, Ci, Co, Lx, k = r.geo[:5]
        assert B <= 5 and Lx <= 300 and max(Ci, Co) <= 256, r.name


def test_every_instance_has_a_row_or_a_reason():
    keys = {r.key for r in W.ROWS}
    x6, f0 = W.x6_instances(), W.f0_instances()
    assert len(x6) == 48 and len([k for k in x6 if k[0] == "x6"]) == 40 and len(f0) == 35
    listed = {u[0] for u in W.UNREACHABLE}
    assert listed <= set(x6 + f0) and all(isinstance(u[1], str) and u[1] for u in W.UNREACHABLE)
    assert not [u for u in W.UNREACHABLE if u[0][0] in ("x6", "wide")], "every x6 instance is reachable without RH_WGRAD_X6_TM"
    missing = [k for k in x6 + f0 if k not in keys and k not in listed]
    assert not missing, [W.fmt_key(k) for k in missing]
    assert not (keys & listed), "an instance listed as unreachable has a row"
    assert keys <= set(x6 + f0), keys - set(x6 + f0)


def test_every_edge_occurs_for_every_kind(L):
    have = {k: set() for k in W.KINDS}
    for r in W.ROWS:
        info = W.instance_info(L, r)
        if W.kind_of(info) is not None:
            have[W.kind_of(info)] |= W.edges(r, info)
    for (kind, e), why in W.NOT_APPLICABLE.items():
        assert e in W.REQUIRED[kind] and why and e not in have[kind], (kind, e)
    missing = [(kind, e) for kind in W.KINDS for e in W.REQUIRED[kind] if (kind, e) not in W.NOT_APPLICABLE and e not in have[kind]]
    assert not missing, missing


def test_a_forced_plane_staging_beyond_the_image_falls_back(L):
    """reach 26 -> p8 = 8 > 7: RH_WGRAD_X6_PLANES=1 still selects the 4-wave kernel by name, with per-column staging."""
    rows = [r for r in W.ROWS if dict(r.env).get(W.PER_CALL[1]) == 1 and r.geo[6] == 13 and r.key[0] == "x6"]
    assert rows and all(r.key[5] == 0 for r in rows)
    for r in rows:
        assert W.instance_info(L, r._replace(geo=r.geo[:6] + (9, (0, 0), False)))[6] == 1, "the same call at reach 18 takes the planes"


def test_unarmed_rows_fall_back_silently(L):
    rows = [r for r in W.ROWS if not r.armed]
    assert rows
    for r in rows:
        assert W.instance_info(L, r)[0] == 0 and W.instance_info(L, r._replace(armed=True))[0] == 1, r.name
    # both x6 tile kinds
    assert {W.instance_info(L, r._replace(armed=True))[1] for r in rows} == {0, 1}


def test_out_of_scope_families_are_reported(L):
    small = W.Row("", (2, 1, 16, 64, 5, 1, 1, (2, 2), False), "", True, 0, (), True, None)
    assert W.instance_info(L, small)[0] == L.lib.rh_conv1d_bwd_weight_kernel_family(C.byref(W.desc(L, small))) == 2
    for r in W.ROWS:
        fam = L.lib.rh_conv1d_bwd_weight_kernel_family(C.byref(W.desc(L, r)))
        assert fam in (0, 1)
        with W.call_env(r):
            assert W.instance_info(L, r)[0] <= fam       # family 1 geometries fall to 0 unarmed / switched off, never the reverse


@pytest.mark.parametrize("armed", (True, False), ids=("armed", "unarmed"))
def test_workspace_query_covers_the_routed_launch(L, armed):
    """rh_conv1d_workspace_bytes (one answer, asked before the caller knows whether the call will be armed) is at least what the
    launch the route chooses demands: the bias scratch, Z > 1 slices of M x C x T partials behind it, and for family 1 the Z x M
    row-sum partials.  The formulas are restated here from W.gemm, not read from the library."""
    for r in W.ROWS:
        row = r._replace(armed=armed)
        info, g = W.instance_info(L, row), W.gemm(row.geo)
        assert info[0] in (0, 1), row.name
        Z = info[7]
        demand = int(L.lib.rh_act_bwd_bias_workspace_bytes(row.geo[2]))
        if Z > 1:
            demand += Z * g["M"] * g["C"] * g["T"] * 4
        if info[0] == 1:
            demand += Z * g["M"] * 4
        assert W.workspace_bytes(L, row) >= demand, (row.name, armed, W.workspace_bytes(L, row), demand)


def _ledger(L):
    lines = ["weight-gradient instance matrix (tests/wgrad_matrix.py; written by tests/test_wgrad_matrix_host.py)", ""]
    for r in W.ROWS:
        info = W.instance_info(L, r)
        sl = W.slicing(info)
        lines.append(f"{r.name:78s} | {W.fmt_key(r.key)} | Z={sl['Z']} {sl['per_z']}/{sl['total']} units of {sl['span']}, {sl['per_b']} per item,"
                     f" tile {sl['rows']}x{sl['cols']} | {', '.join(sorted(W.edges(r, info)))}")
    keys = {r.key for r in W.ROWS}
    lines += ["", f"{len(W.ROWS)} rows; {len(keys & set(W.x6_instances()))} of the {len(W.x6_instances())} x6 instances and "
                  f"{len(keys & set(W.f0_instances()))} of the {len(W.f0_instances())} f32-input instances run",
              "unreachable instances: " + ("none" if not W.UNREACHABLE else "")]
    lines += [f"  {W.fmt_key(u[0])}: {u[1]}" for u in W.UNREACHABLE]
    lines += ["edges that do not exist:"] + [f"  {kind}, {e}: {why}" for (kind, e), why in sorted(W.NOT_APPLICABLE.items())]
    return "\n".join(lines) + "\n"


def test_ledger_is_current(L):
    """The committed ledger is what the table and the planner give today (this test writes nothing)."""
    assert os.path.exists(LEDGER) and open(LEDGER).read() == _ledger(L), \
        "profiles/wgrad_instance_matrix.txt is stale: write it again with `python tests/test_wgrad_matrix_host.py`"


if __name__ == "__main__":     # writes the ledger
    import sys
    sys.path.insert(0, ROOT)
    from rave_amd import _lib
    W.assert_default_planner_env()
    with open(LEDGER, "w") as f:
        f.write(_ledger(_lib))
