"""Host-only proof that tests/conv2d_matrix.py covers the 2-D convolution kernels: every row launches exactly the instance it names
(a change that re-routes a geometry fails here and must update the table), every instance has a row or a reason, every listed edge
occurs for every kernel it exists for, the silent fallbacks and the fused-derivative paths are pinned by key, and the rows stay small.
No GPU: rh_conv2d_instance_info is a pure function of the descriptor, the flags and the per-call switches, answered by the selection
and planning code the launch itself runs.  tests/test_gpu_conv2d_matrix.py runs the same rows on the GPU."""
import ctypes as C
import os
import re

import pytest

import conv2d_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = os.path.join(ROOT, "profiles", "conv2d_instance_matrix.txt")
CSRC = os.path.join(ROOT, "rave_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    from rave_amd import _lib
    M.assert_default_planner_env()
    return _lib


@pytest.mark.parametrize("row", M.ROWS, ids=[r.name for r in M.ROWS])
def test_row_launches_its_key(L, row):
    info = M.instance_info(L, row)
    assert M.key_of(info, row.which) == row.key, (row.name, M.fmt_key(M.key_of(info, row.which)), M.fmt_key(row.key))
    pl = M.plan(info, row.which)
    d = M.desc(L, row)
    if row.which < 2:
        # the older diagnostic agrees where both answer: the family, and the x6 tile plan (it assumes armed ranges and an unfused call)
        out = (C.c_int64 * 16)()
        with M.call_env(row):
            L.check(L.lib.rh_conv2d_plan_info(C.byref(d), row.which, out), "plan_info")
        if row.armed and not (row.which == 1 and row.act):
            assert out[0] == pl["family"], (tuple(out), info)
        if info[0] == 0:
            assert tuple(out[:16]) == (1,) + info[1:4] + (pl["TR"], pl["TQ"], pl["nb"], pl["lds"], pl["gx"] * pl["gy"] * pl["gz"], pl["PH"],
                                                       pl["PW"], pl["nb"] * pl["PH"] * pl["PW"], out[12], pl["phases"], pl["tiles_r"],
                                                       pl["tiles_q"]), (tuple(out), info)
    else:
        with M.call_env(row):
            fam = L.lib.rh_conv2d_bwd_weight_kernel_family(C.byref(d))
        assert pl["family"] <= fam and not pl["short"]
        if row.armed and row.ws:
            assert pl["family"] == fam
        full = int(L.lib.rh_conv2d_workspace_bytes(C.byref(d)))
        assert pl["ws_used"] + pl["bias_ws"] <= M.workspace_bytes(L, row) <= full
        assert pl["ws_used"] == (pl["Z"] * M.numels(row.geo)[2] * 4 if pl["Z"] > 1 else 0)


def test_rows_are_small():
    for r in M.ROWS:
        assert r.geo[0] <= M.MAX_B and max(r.geo[1:3]) <= M.MAX_CH and max(M.numels(r.geo)) <= M.MAX_NUMEL and M.valid(r.geo), r.name


def test_the_inventory_is_the_code():
    """The instance lists of conv2d_matrix are what the sources instantiate."""
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("conv2d_x6.hip", "conv2d_f32.hip", "wgrad2d_x6.hip", "conv2d_smallm.hip",
                                                           "conv2d_smallc.hip")}
    # conv2d_x6.hip: the RH_C2X_CASE list, less the case of the bf16 comparison build (#if !RH_X6_F16)
    x6 = re.sub(r"#if !RH_X6_F16.*?#endif", "", src["conv2d_x6.hip"], flags=re.S)
    cases = {tuple(map(int, m)) for m in re.findall(r"RH_C2X_CASE\((\d), (\d), (\d)\)", x6)}
    assert cases == set(M.X6_TILES) and len(cases) == 10
    tiles = {tuple(map(int, m)) for m in re.findall(r"go2<(\d), (\d), (\d), (\d)>", src["conv2d_f32.hip"])}
    assert tiles == {tuple(map(int, m)) for m in re.findall(r"launch_w2<(\d), (\d), (\d), (\d)>", src["conv2d_f32.hip"])} == set(M.F0_TILES)
    assert set(re.findall(r"launch_w2_dma<(\d)>\(p", src["conv2d_f32.hip"])) == {"1", "2", "4"}
    assert len(M.NO_DMA) == len(re.search(r"enum \{ kDma = 0,([^}]*)\}", src["conv2d_f32.hip"]).group(1).split(",")) + 1
    assert set(re.findall(r"w2x_go<(\d), (\d)>", src["wgrad2d_x6.hip"])) == {("3", "2"), ("3", "1"), ("6", "1")}
    assert set(re.findall(r"smallm_go<(\d), (\d)>", src["conv2d_smallm.hip"])) == {("9", "1"), ("9", "0"), ("3", "1"), ("3", "0")}
    assert set(re.findall(r"conv2d_smallm_kernel<KH, (\d), FLIP>", src["conv2d_smallm.hip"])) == {"1", "2", "4"}
    assert set(re.findall(r"conv2d_smallc_fwd_kernel<(\d)>", src["conv2d_smallc.hip"])) == {"9", "3"}
    inst = M.instances()
    assert len(inst) == len(set(inst)) == 20 + 16 + 4 + 3 + 3 + 12 + 2


def test_every_instance_has_a_row_or_a_reason():
    keys = {r.key for r in M.ROWS}
    inst = set(M.instances())
    listed = {u[0] for u in M.UNREACHABLE}
    assert listed <= inst and all(isinstance(u[1], str) and u[1] for u in M.UNREACHABLE)
    missing = [k for k in M.instances() if k not in keys and k not in listed]
    assert not missing, [M.fmt_key(k) for k in missing]
    assert not (keys & listed), "an instance listed as unreachable has a row"
    assert keys <= inst, keys - inst


def test_every_edge_occurs_for_every_kernel(L):
    have = {k: set() for k in M.KERNELS}
    for r in M.ROWS:
        info = M.instance_info(L, r)
        have[M.kernel_of(info)] |= M.edges(r, info)
    for (kind, e), why in M.NOT_APPLICABLE.items():
        assert e in M.REQUIRED[kind] and why and e not in have[kind], (kind, e)
    missing = [(kind, e) for kind in M.KERNELS for e in M.REQUIRED[kind] if (kind, e) not in M.NOT_APPLICABLE and e not in have[kind]]
    assert not missing, missing


def _twin(L, row, **kw):
    return M.kernel_of(M.instance_info(L, row._replace(**kw)))


def test_fallbacks_are_pinned_by_key(L):
    f0 = ("dma", "igemm", "wdma", "wgrad")
    plain = [r for r in M.ROWS if not r.env]
    # ranges unarmed -> family 0, for a convolution and for the weight gradient
    for which, fam1 in ((0, "x6"), (1, "x6"), (2, "wx6")):
        rows = [r for r in plain if r.which == which and not r.armed and r.key[0] in f0 and _twin(L, r, armed=True, ws=True) == fam1]
        assert rows, f"no unarmed row of an x6-eligible geometry for which = {which}"
    # workspace withheld -> family 0
    assert any(r.which == 2 and r.armed and not r.ws and r.key[0] in f0 and _twin(L, r, ws=True) == "wx6" for r in plain)
    # C % 16 != 0 -> family 0, on both of its kernels; a patch too large for the DMA staging -> conv2d_igemm_kernel
    for kern in ("dma", "igemm"):
        assert any(r.which < 2 and r.key[0] == kern and (r.geo[1] if r.which == 0 else r.geo[2]) % 16 for r in plain), kern
    # ... where plan2_dma itself says that the patch is why it declined (more than 64 * kNI floats even at TR = 1, TQ = 16)
    big = [r for r in M.ROWS if r.key[0] == "igemm" and not r.act and M.plan(M.instance_info(L, r), r.which)["no_dma"] == 3]
    assert big, "no row leaves conv2d_dma_kernel because of the patch size"
    for r in big:
        pl = M.plan(M.instance_info(L, r), r.which)
        k, s, dil = r.geo[5:8]
        is_ = s if r.which == 0 else (1, 1)
        span = [(k[i] - 1) * dil[i] // (1 if r.which == 0 else s[i]) for i in (0, 1)]
        if r.which == 0:
            assert (span[0] + 1) * (15 * is_[1] + span[1] + 1) > 1280, r.name
    # every way into conv2d_igemm_kernel that the default planner has
    assert {M.plan(M.instance_info(L, r), r.which)["no_dma"] for r in M.ROWS if r.key[0] == "igemm"} >= {1, 3, 4}


def test_fused_derivative_rows(L):
    """act = LEAKY with y on the backward entry points: no caller in rave_amd.ops, still public ABI."""
    dgrad = {r.key for r in M.ROWS if r.which == 1 and r.act}
    wgrad = {r.key for r in M.ROWS if r.which == 2 and r.act and r.bias}
    assert len(dgrad) >= 2 and all(k[0] == "igemm" for k in dgrad), dgrad
    assert len(wgrad) >= 2 and all(k[0] == "wgrad" for k in wgrad), wgrad


def test_static_switches_refuse(monkeypatch):
    monkeypatch.setenv("RH_CONV2D_NODMA", "1")
    with pytest.raises(AssertionError):
        M.assert_default_planner_env()


def _ledger(L):
    lines = ["2-D convolution instance matrix (tests/conv2d_matrix.py; written by tests/test_conv2d_matrix_host.py)", ""]
    for r in M.ROWS:
        info = M.instance_info(L, r)
        pl = M.plan(info, r.which)
        if r.which < 2:
            p = (f"TR={pl['TR']} TQ={pl['TQ']} nb={pl['nb']} patch {pl['PH']}x{pl['PW']} ck={pl['ck']} phases={pl['phases']} "
                 f"grid {pl['gx']}x{pl['gy']}x{pl['gz']} lds={pl['lds']}")
        else:
            p = (f"{pl['TR']}x{pl['TQ']} Z={pl['Z']} chunks_per_z={pl['chunks_per_z']} of {pl['total']} groups={pl['groups']} nc_max={pl['nc_max']} "
                 f"lds={pl['lds']} ws={pl['ws_used']}+{pl['bias_ws']} of {M.workspace_bytes(L, r)}")
        lines.append(f"{r.name:74s} | {M.fmt_key(r.key)} | {p} | {', '.join(sorted(M.edges(r, info)))}")
    keys = {r.key for r in M.ROWS}
    lines += ["", f"{len(M.ROWS)} rows; {len(keys & set(M.instances()))} of the {len(M.instances())} instances run", "unreachable instances:"]
    lines += [f"  {M.fmt_key(u[0])}: {u[1]}" for u in M.UNREACHABLE]
    lines += ["edges that do not exist:"] + [f"  {kind}, {e}: {why}" for (kind, e), why in sorted(M.NOT_APPLICABLE.items())]
    return "\n".join(lines) + "\n"


def test_ledger_is_current(L):
    """The committed ledger is what the table and the planner give today (this test writes nothing)."""
    assert os.path.exists(LEDGER) and open(LEDGER).read() == _ledger(L), \
        "profiles/conv2d_instance_matrix.txt is stale: write it again with `python tests/test_conv2d_matrix_host.py`"


if __name__ == "__main__":     # writes the ledger
    import sys
    sys.path.insert(0, ROOT)
    from rave_amd import _lib
    M.assert_default_planner_env()
    with open(LEDGER, "w") as f:
        f.write(_ledger(_lib))
