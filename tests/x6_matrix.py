"""The instance matrix of conv_x6_kernel (csrc/conv_x6_kernel.inc): one row per direct C-ABI call, with the template instance
it must launch (a plain helper module, no fixtures; importing it needs no GPU).

conv_x6_kernel is ~500 template instances: 30 tile shapes (input stride IS 1 / 2 / 4 x the ten (tm, tn, wm) of conv_x6.hip:
RH_X6_SHAPES) x 12 (input LeakyReLU, epilogue) modes, 18 more virtual-row modes for IS == 1, tm >= 2, and four ways of handling
K.  The host planner (conv_x6.hip: plan_x6) picks one from the geometry; ``rh_conv1d_plan_info`` answers "which one" on the host.
``ROWS`` is the smallest set of calls found (by querying that function over small geometries) that reaches every instance the
ABI can reach, every K mode and the column / row edges of the tile addressing; tests/test_x6_matrix_host.py proves that from the
planner alone and tests/test_gpu_x6_matrix.py runs every row against f64.

Instance key = (which, IS, tm, tn, wm, leaky, epi, vs, multiphase, kmode):
  which       0 = rh_conv1d_fwd_f32, 1 = rh_conv1d_bwd_data_f32
  IS          input stride of the fragment layout (1; 2 / 4 = forward of a strided conv, data gradient of a transposed one)
  tm, tn, wm  32-row tiles per wave, 32-column tiles per wave, waves along the rows
  leaky       LeakyReLU fused on the input (forward only)
  epi         OPERAND mode: bit 0 bias, 1 activation derivative (data gradient of an act-leaky conv), 2 add, 3 output LeakyReLU
  vs          0, or 2 / 4 = virtual rows (forward of a transposed conv / data gradient of a strided one as s * M rows)
  multiphase  the same geometries run as s output phases of one launch (grid z) instead
  kmode       "unsplit" | "combine" (2 .. RH_X6_COMBINE slices, arrival counters + x6_combine) | "finalize" (more slices: the
              kernel runs with epilogue 0 and rh_splitk_finalize_launch applies the operands) | "nows" (a split was planned
              but no usable workspace was offered: the call runs unsplit)
``kernel_epi(key)`` is the EPI template argument of the instance that runs (rh_conv_launch_x6).
"""
import ctypes as C
import os
from collections import namedtuple

KMODES = ("unsplit", "combine", "finalize", "nows")
Key = namedtuple("Key", "which IS tm tn wm leaky epi vs multiphase kmode")
# geo = (B, Cin, Cout, L, k, stride, dilation, (pad_left, pad_right), transposed); L = length of the conv's INPUT x
# ops = flags: "L" LeakyReLU(0.2) on the input, "b" bias, "a" residual / add, "o" output LeakyReLU(0.1)
# ws = a workspace of rh_conv1d_*_workspace_bytes is offered; combine = RH_X6_COMBINE for the call (None = unset: 8)
# key = the Key the call must launch, or None = the geometry must plan to family 0 (f32-input MFMA kernels)
Row = namedtuple("Row", "name which geo ops ws combine key")

SLOPE, OUT_SLOPE = 0.2, 0.1
ONCE_PER_PROCESS = ("RH_X6_TN", "RH_X6_SPLIT_BELOW", "RH_X6_SPLIT_TARGET", "RH_X6_VROWS")
SHAPES = [(1, 2, 1), (2, 2, 1), (3, 2, 1), (1, 2, 2), (2, 2, 2), (3, 2, 2), (2, 1, 1), (3, 1, 1), (2, 1, 2), (3, 1, 2)]   # RH_X6_SHAPES


def assert_default_planner_env():
    """The planner reads these once per process: a table pinned under one of them describes another planner."""
    for k in ONCE_PER_PROCESS:
        assert k not in os.environ, f"{k} is set: the instance matrix is pinned for the default planner"
    assert os.environ.get("RH_CONV_X6", "1") != "0", "RH_CONV_X6=0 is set: no call takes conv_x6_kernel"


def epi_instantiated(IS, tm, leaky, epi):
    """conv_params.hpp: rh_x6_epi_instantiated (== the RH_X6_E list of x6_launch), restated."""
    m, v = epi & 15, epi >> 4
    if v:
        if IS != 1 or tm < 2 or v > 2:
            return False
        return m in ((0, 1, 5) if leaky else (0, 1, 2, 4, 5, 6))
    return m in ((0, 1, 4, 5) if leaky else (0, 1, 2, 4, 5, 6, 9, 13))


def instances():
    """Every (IS, tm, tn, wm, leaky, kernel epi) x6_launch instantiates."""
    out = []
    for IS in (1, 2, 4):
        for tm, tn, wm in SHAPES:
            for leaky in (False, True):
                for epi in range(48):
                    if epi_instantiated(IS, tm, leaky, epi):
                        out.append((IS, tm, tn, wm, leaky, epi))
    return out


def out_len(geo):
    B, Ci, Co, L, k, s, dil, pad, tr = geo
    if tr:
        return (L - 1) * s - 2 * pad[0] + k
    return (L + pad[0] + pad[1] - dil * (k - 1) - 1) // s + 1


def operand_mode(row):
    has = lambda f: f in row.ops
    if row.which == 0:
        return (1 if has("b") else 0) | (4 if has("a") else 0) | (8 if has("o") else 0)
    return (2 if has("L") else 0) | (4 if has("a") else 0)


def desc(L, row):
    """``L`` = rave_amd._lib."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    return L.ConvDesc(batch=B, c_in=Ci, c_out=Co, l_in=Lx, l_out=out_len(row.geo), kernel=k, stride=s, dilation=dil,
                      pad_left=pad[0], transposed=int(tr), groups=1, inner=1, in_valid=0, act=1 if "L" in row.ops else 0,
                      act_slope=SLOPE, out_act=1 if "o" in row.ops else 0, out_slope=OUT_SLOPE)


def plan_info(L, row):
    out = (C.c_int32 * 8)()
    L.check(L.lib.rh_conv1d_plan_info(C.byref(desc(L, row)), row.which, int("b" in row.ops and row.which == 0), int("a" in row.ops), out),
            "plan_info")
    return tuple(out)


def workspace_bytes(L, row):
    d = desc(L, row)
    fn = L.lib.rh_conv1d_fwd_workspace_bytes if row.which == 0 else L.lib.rh_conv1d_bwd_data_workspace_bytes
    return int(fn(C.byref(d)))


def _phases(k, s, pad):
    """conv_host.hip: build_plan / phases: first offset and number of taps of each output phase."""
    bases, ntaps = [], []
    for ph in range(s):
        r0 = (ph + pad) % s
        bases.append((ph + pad - r0) // s)
        ntaps.append(len(range(r0, k, s)))
    return bases, ntaps


def _cdiv(a, b):
    return -(-a // b)


def tile_geometry(row, info):
    """The tile fields plan_x6 derives for the plan ``info`` reports (conv_host.hip: build_plan, conv_x6.hip: plan_x6 / shape),
    restated; cross-checked against the workgroup count of ``info`` by derive_key."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    fam, tm, tn, wm, ks, IS, vs, wgs = info
    lo = out_len(row.geo)
    g = dict(B=B, ks=ks, l_out=lo)
    phased = False
    if row.which == 0:
        Cc, M, out_row = Ci, Co, lo
        if not tr:
            rows, minoff, maxoff = lo, -pad[0], (k - 1) * dil - pad[0]
        else:
            phased, rows = True, _cdiv(lo, s)
    else:
        Cc, M, out_row = Co, Ci, Lx
        if tr:
            rows, minoff, maxoff = Lx, -pad[0], k - 1 - pad[0]
        elif s == 1:
            rows, minoff, maxoff = Lx, pad[0] - (k - 1) * dil, pad[0]
        else:
            phased, rows = True, _cdiv(Lx, s)
    nphase, Mr, ncols = 1, M, rows
    if phased:
        bases, ntaps = _phases(k, s, pad[0])
        if vs:
            phstar = next((ph for ph in range(s) if bases[ph] == bases[0] + 1), 0)
            M, ncols = M * s, rows + (1 if phstar else 0)
            minoff, maxoff = bases[0] - max(ntaps) + 1, bases[0]
        else:
            nphase = s
            minoff, maxoff = min(b - n + 1 for b, n in zip(bases, ntaps)), max(bases)
        span = max(ntaps) - 1
    elif IS > 1:
        span = _cdiv(k, IS) - 1
    else:
        span = maxoff - minoff
    Mp = (M + 31) & ~31
    wn = 4 // wm
    BM, BN = 32 * tm * wm, 32 * tn * wn
    bnl = BN
    if ncols < BN:
        bnl = 32
        while bnl < ncols:
            bnl <<= 1
    nb = BN // bnl
    tiles_per_b = _cdiv(ncols, bnl)
    g.update(C=Cc, M=M, Mr=Mr, Mp=Mp, out_row=out_row, ncols=ncols, nphase=nphase, span=span, minoff=minoff, maxoff=maxoff, BM=BM, BN=BN,
             bnl=bnl, nb=nb, tiles_per_b=tiles_per_b, col_tiles=_cdiv(B, nb) * tiles_per_b, row_tiles=_cdiv(Mp, BM),
             lds_P=nb * (bnl + span), nq=3 if wn * tn == 8 else 2)
    g["tiles"] = g["col_tiles"] * g["row_tiles"] * nphase
    # scratch of a split launch (plan_x6: part_bytes): whole register tiles, or the output's layout for the finalize pass
    g["part_bytes"] = max(ks * g["tiles"] * BM * BN * 4, ks * B * Mr * out_row * 4) if ks > 1 else 0
    return g


def derive_key(L, row):
    """The Key of the instance the call of ``row`` launches, by the rules of rh_conv_launch_x6; None = not family 1."""
    assert_default_planner_env()
    info = plan_info(L, row)
    if info[0] != 1:
        return None
    fam, tm, tn, wm, ks, IS, vs, wgs = info
    g = tile_geometry(row, info)
    assert g["tiles"] * ks == wgs, (row.name, "the restated tile geometry disagrees with the planner", g, info)
    assert 2 * g["lds_P"] <= 256 * g["nq"], (row.name, g)
    if ks == 1:
        kmode = "unsplit"
    elif not row.ws or workspace_bytes(L, row) < g["part_bytes"]:
        kmode = "nows"
    elif ks <= (8 if row.combine is None else row.combine):
        kmode = "combine"
    else:
        kmode = "finalize"
    return Key(row.which, IS, tm, tn, wm, row.which == 0 and "L" in row.ops, operand_mode(row), vs, g["nphase"] > 1, kmode)


def kernel_epi(key):
    """EPI template argument of the conv_x6_kernel instance that runs (rh_conv_launch_x6)."""
    return (0 if key.kmode == "finalize" else key.epi) | {0: 0, 2: 16, 4: 32}[key.vs]


def edges(row, info):
    """Names of the column / row edges of the tile addressing this row sits on (``info`` = its plan)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    g = tile_geometry(row, info)
    e = set()
    if g["ncols"] > g["bnl"] and g["ncols"] % g["bnl"]:
        e.add("ragged last column tile")
    if min(B, g["nb"]) > 1:                      # batch items are in fact folded into one tile
        e.add("nb > 1")
        if B > g["nb"] and B % g["nb"]:          # ... and the last tile holds fewer of them than the others
            e.add("B % nb != 0")
    if g["ncols"] == 1:
        e.add("ncols == 1")
    if g["ncols"] == g["bnl"] - 1:
        e.add("ncols == bnl - 1")
    if g["ncols"] == g["bnl"] + 1:
        e.add("ncols == bnl + 1")
    if g["M"] < g["Mp"]:
        e.add("M < Mp")
    if info[3] == 2 and g["Mp"] % g["BM"]:
        e.add("partial last row tile at wm == 2")
    if pad[0] > 0 and pad[1] == 0:
        e.add("causal padding")
    if pad[0] > -g["minoff"] or pad[0] > (k - 1) * dil:
        e.add("padding beyond the left halo")
    # the LDS bound 2 * x6_P <= 256 * nq: one more dilation step (IS == 1) / tap group (IS > 1) would not fit
    step = (k - 1) if info[5] == 1 else 1
    phased = s > 1 and info[5] == 1
    if not phased and step > 0 and 2 * g["nb"] * (g["bnl"] + g["span"] + step) > 256 * g["nq"]:
        e.add("largest staged row that fits LDS")
    return e


def seed(name):
    """Python's hash() is salted per process: a plain checksum of the row's name."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def fmt_key(key):
    if key is None:
        return "family 0 (f32-input MFMA kernels)"
    return (f"{'fwd' if key.which == 0 else 'dgrad'} IS={key.IS} tile={key.tm}{key.tn}{key.wm} {'leaky' if key.leaky else 'plain'} "
            f"epi={key.epi:2d} vs={key.vs} {'phases' if key.multiphase else 'single'} {key.kmode} -> kernel epi {kernel_epi(key)}")


def _name(which, geo, ops, ws, combine):
    B, Ci, Co, Lx, k, s, dil, pad, tr = geo
    return (f"{'fwd' if which == 0 else 'dgrad'} {'convT' if tr else 'conv'}{f' s{s}' if s > 1 else ''} {Ci}->{Co} k{k}"
            f"{f' d{dil}' if dil > 1 else ''} B{B} L{Lx} p{pad[0]},{pad[1]}{f' [{ops}]' if ops else ''}{'' if ws else ' no-ws'}"
            f"{f' combine={combine}' if combine is not None else ''}")


# (which, geo, ops, ws, combine, key): found with tests/x6_matrix_search.py (it asks rh_conv1d_plan_info over small geometries and
# prints the cheapest rows of a wanted key / edge), one query per condition of tests/test_x6_matrix_host.py; the first nine are
# layer-like stride-1 shapes with B > 1 added by hand.  The GPU time allows about a third of the (shape, mode) pairs: operand modes
# are exhaustive per IS (and per vs) on one shape, and every tile shape runs the plain modes 0 and 5 and the derivative mode 2
# (test_x6_matrix_host.py: test_every_shape_runs_the_plain_and_derivative_modes); the edges are not thinned.
# Stride-1 tile shapes are mostly reached through the transposed / strided geometries (virtual rows or output phases): they run
# the same IS == 1 instances.  The last three are over the LDS bound and must NOT plan to the shape of their sibling.
_TABLE = [
    (0, (3, 96, 96, 257, 3, 1, 9, (9, 9), False), 'L', True, None, (0, 1, 3, 1, 1, True, 0, 0, False, 'combine')),
    (1, (3, 96, 96, 257, 3, 1, 9, (9, 9), False), 'La', True, None, (1, 1, 3, 1, 1, False, 6, 0, False, 'combine')),
    (0, (5, 64, 128, 33, 3, 1, 1, (2, 0), False), 'Lba', True, None, (0, 1, 2, 1, 2, True, 5, 0, False, 'combine')),
    (1, (3, 64, 192, 65, 5, 1, 2, (4, 4), False), 'L', True, None, (1, 1, 2, 1, 1, False, 2, 0, False, 'combine')),
    (0, (2, 32, 64, 129, 7, 1, 1, (3, 3), False), 'b', True, None, (0, 1, 2, 1, 1, False, 1, 0, False, 'unsplit')),
    (1, (5, 160, 32, 31, 3, 1, 1, (2, 0), False), 'a', True, None, (1, 1, 1, 2, 2, False, 4, 0, False, 'unsplit')),
    (0, (9, 384, 768, 32, 3, 1, 1, (1, 1), False), 'Lba', True, 2, (0, 1, 3, 1, 2, True, 5, 0, False, 'finalize')),
    (1, (9, 384, 768, 32, 3, 1, 1, (1, 1), False), 'La', True, 2, (1, 1, 3, 1, 2, False, 6, 0, False, 'finalize')),
    (0, (3, 192, 96, 64, 3, 1, 3, (6, 0), False), 'Lba', False, None, (0, 1, 3, 1, 1, True, 5, 0, False, 'nows')),
    (0, (2, 16, 32, 300, 3, 1, 64, (64, 64), False), 'Lb', True, None, (0, 1, 1, 2, 1, True, 1, 0, False, 'unsplit')),
    (0, (1, 16, 144, 127, 1, 1, 1, (2, 0), False), 'ba', True, None, (0, 1, 1, 2, 2, False, 5, 0, False, 'unsplit')),
    (0, (1, 64, 144, 1, 3, 1, 1, (1, 1), False), 'L', True, None, (0, 1, 1, 2, 2, True, 0, 0, False, 'combine')),
    (1, (1, 144, 64, 1, 3, 1, 1, (1, 1), False), 'L', False, None, (1, 1, 1, 2, 2, False, 2, 0, False, 'nows')),
    (0, (1, 64, 48, 1, 3, 1, 1, (1, 1), False), '', True, 1, (0, 1, 2, 1, 1, False, 0, 0, False, 'finalize')),
    (0, (1, 16, 48, 63, 2, 1, 128, (130, 0), False), 'b', True, None, (0, 1, 2, 1, 1, False, 1, 0, False, 'unsplit')),
    (0, (1, 16, 128, 49157, 3, 1, 65, (65, 65), False), 'b', True, None, (0, 1, 2, 1, 2, False, 1, 0, False, 'unsplit')),
    (0, (1, 16, 128, 49157, 3, 1, 65, (64, 64), False), 'b', True, None, (0, 1, 2, 1, 2, False, 1, 0, False, 'unsplit')),
    (0, (1, 64, 48, 49155, 17, 1, 1, (18, 0), False), '', True, None, (0, 1, 2, 2, 1, False, 0, 0, False, 'combine')),
    (0, (1, 16, 48, 98307, 1, 1, 1, (2, 0), False), 'ba', True, None, (0, 1, 2, 2, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 64, 128, 8325, 17, 1, 1, (18, 0), False), '', True, None, (0, 1, 2, 2, 2, False, 0, 0, False, 'combine')),
    (0, (1, 16, 128, 49157, 3, 1, 64, (64, 64), False), 'b', True, None, (0, 1, 2, 2, 2, False, 1, 0, False, 'unsplit')),
    (1, (1, 176, 16, 1, 1, 1, 1, (0, 0), False), 'L', True, None, (1, 1, 3, 1, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 64, 96, 17016, 17, 1, 1, (8, 8), False), 'Lb', True, None, (0, 1, 3, 2, 1, True, 1, 0, False, 'combine')),
    (0, (1, 64, 176, 8325, 17, 1, 1, (18, 0), False), '', True, None, (0, 1, 3, 2, 2, False, 0, 0, False, 'combine')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'a', True, None, (0, 1, 1, 2, 1, False, 4, 0, True, 'unsplit')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'bo', True, None, (0, 1, 1, 2, 1, False, 9, 0, True, 'unsplit')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'bao', True, None, (0, 1, 1, 2, 1, False, 13, 0, True, 'unsplit')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'Lb', True, None, (0, 1, 1, 2, 1, True, 1, 0, True, 'unsplit')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'La', True, None, (0, 1, 1, 2, 1, True, 4, 0, True, 'unsplit')),
    (0, (1, 16, 8, 31, 2, 2, 1, (0, 0), True), 'Lba', True, None, (0, 1, 1, 2, 1, True, 5, 0, True, 'unsplit')),
    (1, (1, 8, 64, 4, 16, 4, 1, (15, 0), False), '', True, None, (1, 1, 1, 2, 1, False, 0, 0, True, 'combine')),
    (1, (1, 8, 64, 2, 5, 2, 1, (0, 3), False), '', True, 1, (1, 1, 1, 2, 1, False, 0, 0, True, 'finalize')),
    (1, (1, 8, 16, 2, 2, 2, 1, (0, 0), False), 'L', True, None, (1, 1, 1, 2, 1, False, 2, 0, True, 'unsplit')),
    (1, (1, 8, 16, 2, 2, 2, 1, (0, 0), False), 'La', True, None, (1, 1, 1, 2, 1, False, 6, 0, True, 'unsplit')),
    (1, (1, 80, 16, 2, 2, 2, 1, (1, 0), False), 'L', True, None, (1, 1, 3, 1, 1, False, 2, 0, True, 'unsplit')),
    (0, (1, 16, 80, 49160, 2, 2, 1, (1, 1), True), 'ba', True, None, (0, 1, 3, 2, 1, False, 5, 0, True, 'unsplit')),
    (0, (1, 16, 32, 1, 2, 2, 1, (0, 0), True), '', True, None, (0, 1, 2, 1, 1, False, 0, 2, False, 'unsplit')),
    (0, (1, 16, 32, 1, 2, 2, 1, (0, 0), True), 'b', True, None, (0, 1, 2, 1, 1, False, 1, 2, False, 'unsplit')),
    (0, (1, 16, 32, 1, 2, 2, 1, (0, 0), True), 'a', True, None, (0, 1, 2, 1, 1, False, 4, 2, False, 'unsplit')),
    (0, (1, 16, 32, 1, 2, 2, 1, (0, 0), True), 'Lb', True, None, (0, 1, 2, 1, 1, True, 1, 2, False, 'unsplit')),
    (1, (1, 32, 16, 2, 2, 2, 1, (0, 0), False), 'La', True, None, (1, 1, 2, 1, 1, False, 6, 2, False, 'unsplit')),
    (0, (1, 16, 64, 1, 2, 2, 1, (0, 0), True), 'Lba', True, None, (0, 1, 2, 1, 2, True, 5, 2, False, 'unsplit')),
    (1, (1, 64, 64, 2, 5, 2, 1, (0, 3), False), 'L', True, None, (1, 1, 2, 1, 2, False, 2, 2, False, 'combine')),
    (1, (1, 32, 16, 196620, 2, 2, 1, (0, 0), False), 'L', True, None, (1, 1, 2, 2, 1, False, 2, 2, False, 'unsplit')),
    (1, (1, 64, 16, 98320, 2, 2, 1, (0, 0), False), 'L', True, None, (1, 1, 2, 2, 2, False, 2, 2, False, 'unsplit')),
    (0, (1, 64, 48, 1, 5, 2, 1, (1, 1), True), 'L', False, None, (0, 1, 3, 1, 1, True, 0, 2, False, 'nows')),
    (0, (1, 16, 96, 1, 2, 2, 1, (0, 0), True), 'ba', True, None, (0, 1, 3, 1, 2, False, 5, 2, False, 'unsplit')),
    (1, (1, 48, 16, 196620, 2, 2, 1, (0, 0), False), 'L', True, None, (1, 1, 3, 2, 1, False, 2, 2, False, 'unsplit')),
    (0, (1, 16, 144, 24600, 2, 2, 1, (1, 1), True), '', True, None, (0, 1, 3, 2, 2, False, 0, 2, False, 'unsplit')),
    (0, (1, 16, 144, 24600, 2, 2, 1, (1, 1), True), 'ba', True, None, (0, 1, 3, 2, 2, False, 5, 2, False, 'unsplit')),
    (0, (1, 16, 16, 1, 4, 4, 1, (0, 0), True), 'b', True, None, (0, 1, 2, 1, 1, False, 1, 4, False, 'unsplit')),
    (0, (1, 16, 16, 1, 4, 4, 1, (0, 0), True), 'a', True, None, (0, 1, 2, 1, 1, False, 4, 4, False, 'unsplit')),
    (0, (1, 16, 16, 1, 4, 4, 1, (0, 0), True), 'Lb', True, None, (0, 1, 2, 1, 1, True, 1, 4, False, 'unsplit')),
    (0, (1, 64, 16, 1, 9, 4, 1, (2, 2), True), 'Lba', False, None, (0, 1, 2, 1, 1, True, 5, 4, False, 'nows')),
    (1, (1, 16, 64, 124, 9, 4, 1, (0, 5), False), 'L', True, None, (1, 1, 2, 1, 1, False, 2, 4, False, 'combine')),
    (1, (1, 16, 16, 4, 4, 4, 1, (0, 0), False), 'La', True, None, (1, 1, 2, 1, 1, False, 6, 4, False, 'unsplit')),
    (0, (1, 16, 80, 65, 4, 4, 1, (0, 0), True), '', True, None, (0, 1, 2, 1, 2, False, 0, 4, False, 'unsplit')),
    (0, (1, 16, 16, 98310, 4, 4, 1, (3, 3), True), '', True, None, (0, 1, 2, 2, 1, False, 0, 4, False, 'unsplit')),
    (0, (1, 16, 64, 24600, 4, 4, 1, (3, 3), True), 'ba', True, None, (0, 1, 2, 2, 2, False, 5, 4, False, 'unsplit')),
    (0, (1, 16, 64, 24600, 4, 4, 1, (3, 3), True), 'L', True, None, (0, 1, 2, 2, 2, True, 0, 4, False, 'unsplit')),
    (0, (1, 64, 24, 1, 9, 4, 1, (2, 2), True), 'ba', True, None, (0, 1, 3, 1, 1, False, 5, 4, False, 'combine')),
    (1, (1, 24, 64, 4, 9, 4, 1, (0, 5), False), '', True, 1, (1, 1, 3, 1, 1, False, 0, 4, False, 'finalize')),
    (1, (1, 48, 64, 4, 9, 4, 1, (0, 5), False), '', True, None, (1, 1, 3, 1, 2, False, 0, 4, False, 'combine')),
    (0, (2, 16, 48, 3, 4, 4, 1, (0, 0), True), 'Lb', True, None, (0, 1, 3, 1, 2, True, 1, 4, False, 'unsplit')),
    (0, (1, 16, 24, 98310, 4, 4, 1, (3, 3), True), '', True, None, (0, 1, 3, 2, 1, False, 0, 4, False, 'unsplit')),
    (1, (1, 96, 16, 98400, 4, 4, 1, (0, 0), False), 'L', True, None, (1, 1, 3, 2, 2, False, 2, 4, False, 'unsplit')),
    (0, (1, 8, 20, 1, 2, 2, 1, (1, 0), False), '', True, None, (0, 2, 1, 2, 1, False, 0, 0, False, 'unsplit')),
    (0, (1, 32, 20, 1, 4, 2, 1, (3, 0), False), 'a', False, None, (0, 2, 1, 2, 1, False, 4, 0, False, 'nows')),
    (0, (1, 32, 20, 1, 34, 2, 1, (33, 0), False), 'ba', True, None, (0, 2, 1, 2, 1, False, 5, 0, False, 'combine')),
    (0, (1, 8, 20, 1, 2, 2, 1, (1, 0), False), 'bo', True, None, (0, 2, 1, 2, 1, False, 9, 0, False, 'unsplit')),
    (0, (1, 8, 20, 1, 2, 2, 1, (1, 0), False), 'bao', True, None, (0, 2, 1, 2, 1, False, 13, 0, False, 'unsplit')),
    (0, (1, 8, 20, 1, 2, 2, 1, (1, 0), False), 'Lb', True, None, (0, 2, 1, 2, 1, True, 1, 0, False, 'unsplit')),
    (0, (1, 8, 20, 1, 2, 2, 1, (1, 0), False), 'La', True, None, (0, 2, 1, 2, 1, True, 4, 0, False, 'unsplit')),
    (1, (1, 20, 8, 1, 2, 2, 1, (0, 0), True), 'L', True, None, (1, 2, 1, 2, 1, False, 2, 0, False, 'unsplit')),
    (1, (1, 20, 32, 1, 4, 2, 1, (1, 0), True), 'La', True, 1, (1, 2, 1, 2, 1, False, 6, 0, False, 'finalize')),
    (1, (1, 20, 8, 1, 2, 2, 1, (0, 0), True), 'La', True, None, (1, 2, 1, 2, 1, False, 6, 0, False, 'unsplit')),
    (0, (1, 32, 144, 1, 4, 2, 1, (3, 0), False), 'b', True, None, (0, 2, 1, 2, 2, False, 1, 0, False, 'combine')),
    (0, (1, 8, 144, 1, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 1, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 144, 8, 31, 2, 2, 1, (3, 0), True), '', True, None, (1, 2, 1, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 144, 8, 1, 2, 2, 1, (0, 0), True), 'L', True, None, (1, 2, 1, 2, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 32, 48, 1, 4, 2, 1, (3, 0), False), '', True, None, (0, 2, 2, 1, 1, False, 0, 0, False, 'combine')),
    (0, (1, 8, 48, 1, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 2, 1, 1, False, 5, 0, False, 'unsplit')),
    (1, (1, 48, 8, 129, 2, 2, 1, (3, 0), True), 'L', True, None, (1, 2, 2, 1, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 8, 128, 1, 2, 2, 1, (1, 0), False), 'Lba', True, None, (0, 2, 2, 1, 2, True, 5, 0, False, 'unsplit')),
    (1, (1, 128, 32, 1, 4, 2, 1, (1, 0), True), '', True, None, (1, 2, 2, 1, 2, False, 0, 0, False, 'combine')),
    (1, (1, 128, 8, 1, 2, 2, 1, (0, 0), True), 'L', True, None, (1, 2, 2, 1, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 8, 48, 196615, 2, 2, 1, (3, 0), False), 'ba', True, None, (0, 2, 2, 2, 1, False, 5, 0, False, 'unsplit')),
    (1, (1, 48, 32, 49157, 34, 2, 1, (35, 0), True), '', True, None, (1, 2, 2, 2, 1, False, 0, 0, False, 'combine')),
    (1, (1, 48, 8, 98309, 2, 2, 1, (3, 0), True), '', True, None, (1, 2, 2, 2, 1, False, 0, 0, False, 'unsplit')),
    (1, (1, 48, 8, 98309, 2, 2, 1, (3, 0), True), 'L', True, None, (1, 2, 2, 2, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 8, 128, 98311, 2, 2, 1, (3, 0), False), 'ba', True, None, (0, 2, 2, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 128, 32, 8327, 34, 2, 1, (35, 0), True), '', True, None, (1, 2, 2, 2, 2, False, 0, 0, False, 'combine')),
    (1, (1, 128, 8, 49157, 2, 2, 1, (3, 0), True), '', True, None, (1, 2, 2, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 128, 8, 49157, 2, 2, 1, (3, 0), True), 'L', True, None, (1, 2, 2, 2, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 8, 80, 1, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 3, 1, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 8, 80, 1, 2, 2, 1, (1, 0), False), 'L', True, None, (0, 2, 3, 1, 1, True, 0, 0, False, 'unsplit')),
    (1, (1, 80, 32, 1, 4, 2, 1, (1, 0), True), 'L', True, None, (1, 2, 3, 1, 1, False, 2, 0, False, 'combine')),
    (0, (1, 8, 176, 1, 2, 2, 1, (1, 0), False), '', True, None, (0, 2, 3, 1, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 8, 176, 1, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 3, 1, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 176, 32, 1, 4, 2, 1, (1, 0), True), 'L', True, None, (1, 2, 3, 1, 2, False, 2, 0, False, 'combine')),
    (0, (1, 8, 80, 196615, 2, 2, 1, (3, 0), False), 'ba', True, None, (0, 2, 3, 2, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 32, 96, 34000, 34, 2, 1, (16, 16), False), 'Lb', True, None, (0, 2, 3, 2, 1, True, 1, 0, False, 'combine')),
    (1, (1, 80, 8, 98309, 2, 2, 1, (3, 0), True), '', True, None, (1, 2, 3, 2, 1, False, 0, 0, False, 'unsplit')),
    (1, (1, 80, 8, 98309, 2, 2, 1, (3, 0), True), 'L', True, None, (1, 2, 3, 2, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 8, 176, 98311, 2, 2, 1, (3, 0), False), 'ba', True, None, (0, 2, 3, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 176, 32, 8327, 34, 2, 1, (35, 0), True), '', True, None, (1, 2, 3, 2, 2, False, 0, 0, False, 'combine')),
    (1, (1, 176, 8, 49157, 2, 2, 1, (3, 0), True), '', True, None, (1, 2, 3, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 176, 8, 49157, 2, 2, 1, (3, 0), True), 'L', True, None, (1, 2, 3, 2, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 16, 20, 1, 8, 4, 1, (7, 0), False), 'b', True, 1, (0, 4, 1, 2, 1, False, 1, 0, False, 'finalize')),
    (0, (1, 16, 20, 1, 8, 4, 1, (7, 0), False), 'a', False, None, (0, 4, 1, 2, 1, False, 4, 0, False, 'nows')),
    (0, (1, 4, 20, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 1, 2, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 4, 20, 1, 4, 4, 1, (3, 0), False), 'bo', True, None, (0, 4, 1, 2, 1, False, 9, 0, False, 'unsplit')),
    (0, (1, 4, 20, 1, 4, 4, 1, (3, 0), False), 'bao', True, None, (0, 4, 1, 2, 1, False, 13, 0, False, 'unsplit')),
    (0, (1, 4, 20, 1, 4, 4, 1, (3, 0), False), 'Lb', True, None, (0, 4, 1, 2, 1, True, 1, 0, False, 'unsplit')),
    (0, (1, 4, 20, 1, 4, 4, 1, (3, 0), False), 'La', True, None, (0, 4, 1, 2, 1, True, 4, 0, False, 'unsplit')),
    (1, (1, 20, 16, 1, 8, 4, 1, (2, 0), True), '', True, None, (1, 4, 1, 2, 1, False, 0, 0, False, 'combine')),
    (1, (1, 20, 4, 1, 4, 4, 1, (0, 0), True), 'L', True, None, (1, 4, 1, 2, 1, False, 2, 0, False, 'unsplit')),
    (1, (1, 20, 4, 1, 4, 4, 1, (0, 0), True), 'La', True, None, (1, 4, 1, 2, 1, False, 6, 0, False, 'unsplit')),
    (0, (1, 16, 144, 1, 8, 4, 1, (7, 0), False), 'b', True, None, (0, 4, 1, 2, 2, False, 1, 0, False, 'combine')),
    (0, (1, 4, 144, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 1, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 144, 4, 31, 4, 4, 1, (5, 0), True), '', True, None, (1, 4, 1, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 144, 4, 1, 4, 4, 1, (0, 0), True), 'L', True, None, (1, 4, 1, 2, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 4, 48, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 2, 1, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 4, 48, 1, 4, 4, 1, (3, 0), False), 'L', True, None, (0, 4, 2, 1, 1, True, 0, 0, False, 'unsplit')),
    (1, (1, 48, 16, 129, 8, 4, 1, (9, 0), True), 'L', True, None, (1, 4, 2, 1, 1, False, 2, 0, False, 'combine')),
    (0, (1, 4, 128, 1, 4, 4, 1, (3, 0), False), '', True, None, (0, 4, 2, 1, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 4, 128, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 2, 1, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 128, 16, 1, 8, 4, 1, (2, 0), True), 'L', True, None, (1, 4, 2, 1, 2, False, 2, 0, False, 'combine')),
    (0, (1, 4, 48, 393231, 4, 4, 1, (5, 0), False), 'ba', True, None, (0, 4, 2, 2, 1, False, 5, 0, False, 'unsplit')),
    (1, (1, 48, 32, 49157, 34, 4, 1, (35, 0), True), '', True, None, (1, 4, 2, 2, 1, False, 0, 0, False, 'combine')),
    (1, (1, 48, 4, 98309, 4, 4, 1, (5, 0), True), '', True, None, (1, 4, 2, 2, 1, False, 0, 0, False, 'unsplit')),
    (1, (1, 48, 4, 98309, 4, 4, 1, (5, 0), True), 'L', True, None, (1, 4, 2, 2, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 4, 128, 196623, 4, 4, 1, (5, 0), False), 'ba', True, None, (0, 4, 2, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 128, 32, 8327, 34, 4, 1, (35, 0), True), '', True, None, (1, 4, 2, 2, 2, False, 0, 0, False, 'combine')),
    (1, (1, 128, 4, 49157, 4, 4, 1, (5, 0), True), '', True, None, (1, 4, 2, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 128, 4, 49157, 4, 4, 1, (5, 0), True), 'L', True, None, (1, 4, 2, 2, 2, False, 2, 0, False, 'unsplit')),
    (0, (1, 4, 80, 1, 4, 4, 1, (3, 0), False), 'Lba', True, None, (0, 4, 3, 1, 1, True, 5, 0, False, 'unsplit')),
    (1, (1, 80, 16, 1, 8, 4, 1, (2, 0), True), '', True, None, (1, 4, 3, 1, 1, False, 0, 0, False, 'combine')),
    (1, (1, 80, 4, 1, 4, 4, 1, (0, 0), True), 'L', True, None, (1, 4, 3, 1, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 4, 176, 1, 4, 4, 1, (3, 0), False), '', True, None, (0, 4, 3, 1, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 4, 176, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 3, 1, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 176, 16, 1, 8, 4, 1, (2, 0), True), 'L', True, None, (1, 4, 3, 1, 2, False, 2, 0, False, 'combine')),
    (0, (1, 4, 80, 393231, 4, 4, 1, (5, 0), False), 'ba', True, None, (0, 4, 3, 2, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 32, 96, 68000, 36, 4, 1, (16, 16), False), 'Lb', True, None, (0, 4, 3, 2, 1, True, 1, 0, False, 'combine')),
    (1, (1, 80, 4, 98309, 4, 4, 1, (5, 0), True), '', True, None, (1, 4, 3, 2, 1, False, 0, 0, False, 'unsplit')),
    (1, (1, 80, 4, 98309, 4, 4, 1, (5, 0), True), 'L', True, None, (1, 4, 3, 2, 1, False, 2, 0, False, 'unsplit')),
    (0, (1, 4, 176, 196623, 4, 4, 1, (5, 0), False), 'ba', True, None, (0, 4, 3, 2, 2, False, 5, 0, False, 'unsplit')),
    (1, (1, 176, 32, 8327, 34, 4, 1, (35, 0), True), '', True, None, (1, 4, 3, 2, 2, False, 0, 0, False, 'combine')),
    (1, (1, 176, 4, 49157, 4, 4, 1, (5, 0), True), '', True, None, (1, 4, 3, 2, 2, False, 0, 0, False, 'unsplit')),
    (1, (1, 176, 4, 49157, 4, 4, 1, (5, 0), True), 'L', True, None, (1, 4, 3, 2, 2, False, 2, 0, False, 'unsplit')),
    # batch folding for real: more items than one tile folds (B > nb > 1) and a last tile with fewer of them (B % nb != 0), for the
    # IS > 1 staging, the virtual-row epilogue and the 64-column wave tile, forward and data gradient, unsplit and split in K
    (0, (9, 32, 20, 5, 4, 2, 1, (3, 0), False), '', True, None, (0, 2, 1, 2, 1, False, 0, 0, False, 'combine')),
    (0, (5, 8, 48, 7, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 2, 1, 1, False, 5, 0, False, 'unsplit')),
    (0, (5, 32, 48, 7, 4, 2, 1, (3, 0), False), 'Lb', True, 1, (0, 2, 2, 1, 1, True, 1, 0, False, 'finalize')),
    (1, (9, 20, 8, 3, 2, 2, 1, (0, 0), True), 'L', True, None, (1, 2, 1, 2, 1, False, 2, 0, False, 'unsplit')),
    (1, (5, 48, 32, 3, 4, 2, 1, (1, 0), True), 'La', True, None, (1, 2, 2, 1, 1, False, 6, 0, False, 'combine')),
    (0, (9, 4, 20, 9, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 1, 2, 1, False, 5, 0, False, 'unsplit')),
    (0, (5, 16, 48, 5, 8, 4, 1, (7, 0), False), 'b', True, None, (0, 4, 2, 1, 1, False, 1, 0, False, 'combine')),
    (1, (9, 20, 16, 2, 8, 4, 1, (2, 0), True), '', True, None, (1, 4, 1, 2, 1, False, 0, 0, False, 'combine')),
    (1, (5, 48, 4, 3, 4, 4, 1, (0, 0), True), 'L', True, None, (1, 4, 2, 1, 1, False, 2, 0, False, 'unsplit')),
    (0, (5, 16, 32, 3, 2, 2, 1, (0, 0), True), 'ba', True, None, (0, 1, 2, 1, 1, False, 5, 2, False, 'unsplit')),
    (0, (5, 64, 32, 3, 4, 2, 1, (1, 1), True), 'Lb', True, None, (0, 1, 2, 1, 1, True, 1, 2, False, 'combine')),
    (1, (5, 32, 64, 6, 2, 2, 1, (0, 0), False), 'L', True, None, (1, 1, 2, 1, 1, False, 2, 2, False, 'combine')),
    (1, (3, 64, 16, 6, 2, 2, 1, (0, 0), False), 'a', True, None, (1, 1, 2, 1, 2, False, 4, 2, False, 'unsplit')),
    (0, (5, 64, 16, 3, 4, 4, 1, (0, 0), True), '', True, None, (0, 1, 2, 1, 1, False, 0, 4, False, 'combine')),
    (0, (3, 16, 32, 3, 4, 4, 1, (0, 0), True), 'ba', True, None, (0, 1, 2, 1, 2, False, 5, 4, False, 'unsplit')),
    (1, (5, 16, 16, 12, 4, 4, 1, (0, 0), False), 'La', True, None, (1, 1, 2, 1, 1, False, 6, 4, False, 'unsplit')),
    (1, (5, 16, 64, 12, 8, 4, 1, (2, 2), False), 'L', True, None, (1, 1, 2, 1, 1, False, 2, 4, False, 'combine')),
    (0, (9, 16, 32, 5, 3, 1, 1, (2, 0), False), 'b', True, None, (0, 1, 1, 2, 1, False, 1, 0, False, 'unsplit')),
    (1, (9, 32, 16, 5, 3, 1, 1, (1, 1), False), 'L', True, None, (1, 1, 1, 2, 1, False, 2, 0, False, 'unsplit')),
    (0, (5, 64, 160, 7, 3, 1, 1, (1, 1), False), 'Lba', True, None, (0, 1, 1, 2, 2, True, 5, 0, False, 'combine')),
    # every tile shape on the plain modes 0 and 5 and on the derivative mode: what the rows above left out
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), '', True, None, (0, 1, 1, 2, 1, False, 0, 0, True, 'unsplit')),
    (0, (1, 16, 8, 1, 2, 2, 1, (0, 0), True), 'ba', True, None, (0, 1, 1, 2, 1, False, 5, 0, True, 'unsplit')),
    (0, (1, 64, 144, 1, 3, 1, 1, (1, 1), False), '', True, None, (0, 1, 1, 2, 2, False, 0, 0, False, 'combine')),
    (0, (1, 16, 32, 1, 2, 2, 1, (0, 0), True), 'ba', True, None, (0, 1, 2, 1, 1, False, 5, 2, False, 'unsplit')),
    (0, (1, 16, 80, 2, 2, 2, 1, (1, 1), True), '', True, None, (0, 1, 3, 1, 1, False, 0, 0, True, 'unsplit')),
    (0, (1, 16, 64, 1, 2, 2, 1, (0, 0), True), 'ba', True, None, (0, 1, 2, 1, 2, False, 5, 2, False, 'unsplit')),
    (0, (1, 16, 176, 1, 1, 1, 1, (0, 0), False), '', True, None, (0, 1, 3, 1, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 8, 144, 1, 2, 2, 1, (1, 0), False), '', True, None, (0, 2, 1, 2, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 8, 80, 1, 2, 2, 1, (1, 0), False), '', True, None, (0, 2, 3, 1, 1, False, 0, 0, False, 'unsplit')),
    (0, (1, 8, 128, 1, 2, 2, 1, (1, 0), False), '', True, None, (0, 2, 2, 1, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 8, 128, 1, 2, 2, 1, (1, 0), False), 'ba', True, None, (0, 2, 2, 1, 2, False, 5, 0, False, 'unsplit')),
    (0, (1, 4, 144, 1, 4, 4, 1, (3, 0), False), '', True, None, (0, 4, 1, 2, 2, False, 0, 0, False, 'unsplit')),
    (0, (1, 4, 48, 1, 4, 4, 1, (3, 0), False), '', True, None, (0, 4, 2, 1, 1, False, 0, 0, False, 'unsplit')),
    (0, (1, 4, 80, 1, 4, 4, 1, (3, 0), False), '', True, None, (0, 4, 3, 1, 1, False, 0, 0, False, 'unsplit')),
    (0, (1, 4, 80, 1, 4, 4, 1, (3, 0), False), 'ba', True, None, (0, 4, 3, 1, 1, False, 5, 0, False, 'unsplit')),
    (0, (1, 16, 48, 63, 2, 1, 129, (130, 0), False), 'b', True, None, None),
    (0, (1, 32, 20, 3, 36, 2, 1, (33, 0), False), 'ba', True, None, None),
    (0, (2, 16, 32, 300, 3, 1, 65, (64, 64), False), 'Lb', True, None, None),
]
ROWS = [Row(_name(w, g, o, ws, c), w, g, o, ws, c, None if k is None else Key(*k)) for w, g, o, ws, c, k in _TABLE]
assert len({r.name for r in ROWS}) == len(ROWS)

# (IS, tm, tn, wm, leaky, kernel epi) x6_launch instantiates but no geometry can select through the C ABI, with the planner's reason.
# None: every operand mode of rh_x6_epi_instantiated is expressible on every tile shape (the tile shape follows the sizes alone,
# the mode the operands alone; the one coupling -- virtual rows need their own instance, plan_x6: epi_ok -- only moves a call
# between two instances that both exist).  tests/test_x6_matrix_host.py proves it by planning every pair.
UNREACHABLE = []
# Operand sets the ABI cannot express at all (so no refusal test exists for them): a LeakyReLU input together with the derivative
# epilogue -- rh_conv_fill_dgrad sets in_act = NONE, rh_conv1d_fwd_f32 sets mul_src = nullptr.
INEXPRESSIBLE = ["derivative epilogue with a LeakyReLU input (conv_host.hip: rh_conv_fill_dgrad / rh_conv1d_fwd_f32)"]
