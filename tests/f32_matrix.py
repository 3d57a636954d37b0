"""The instance matrix of the f32-input MFMA forward / data-gradient kernels ("family 0": csrc/conv_igemm_dma.hip, csrc/conv_igemm.hip):
one row per direct C-ABI call with NO input range slot armed, with the kernel instance it must launch (a plain helper module, no
fixtures; importing it needs no GPU).

Family 0 is 24 ``conv_igemm_dma_kernel`` instances (4 tile shapes x LEAKY x {VEC, VEC + CTAIL, element-wise + CTAIL}), 4
``conv_igemm_kernel`` instances (Snake inputs, descriptors beyond 2 GiB, DMA stages beyond 160 KiB of LDS) and the two split-K
finalize kernels.  ``rh_conv1d_f32_instance_info`` answers "which one" on the host from the planning code the launch itself runs.
``ROWS`` was found by tests/f32_matrix_search.py; tests/test_f32_matrix_host.py proves from the planner alone that it reaches every
instance, K mode and tile edge, and tests/test_gpu_f32_matrix.py runs every row against f64.

Key = (which, kernel, TM, TN, WM, WN, leaky, vec, ctail, kmode, multiphase, inner):
  which       0 = rh_conv1d_fwd_f32, 1 = rh_conv1d_bwd_data_f32
  kernel      1 = conv_igemm_dma_kernel, 0 = conv_igemm_kernel
  TM .. WN    32-row / 32-column tiles per wave, waves along the rows / columns
  leaky, vec, ctail   template arguments of the DMA kernel (False for the synchronous one)
  kmode       "unsplit" | "finalize" (K slices + splitk_finalize_kernel) | "finalize4" (+ splitk_finalize4_kernel) | "nows" (a
              split was planned, no workspace was offered: the call runs unsplit)
  multiphase  more than one output phase in grid z (transposed forward, strided data gradient)
  inner       the (k,1) period-fold form with inner > 1
"""
import ctypes as C
import os
from collections import namedtuple

KMODES = ("unsplit", "finalize", "finalize4", "nows")
Key = namedtuple("Key", "which kernel TM TN WM WN leaky vec ctail kmode multiphase inner")
# geo = (B, Cin, Cout, L, k, stride, dilation, (pad_left, pad_right), transposed, inner, in_valid); L = positions of the conv's INPUT
#       x (rows of ``inner`` elements); in_valid = elements of a memory row of x (0 = all L * inner; less = the fold's zero padding)
# ops = flags: "L" LeakyReLU(0.2) / "S" Snake on the input (data gradient: their derivative), "b" bias, "a" residual / add,
#       "o" output LeakyReLU(0.1)
# align = 16 or 4: every data pointer of the call is carved at that alignment; ws = a workspace of rh_conv1d_*_workspace_bytes is offered
Row = namedtuple("Row", "name which geo ops align ws key")
Info = namedtuple("Info", "family kernel TM TN WM WN leaky vec ctail lds_fallback ck total_chunks ks chunks_per_slice finalize nb bnl "
                          "tiles_per_b nphase inner pitch segs lds gx gy gz maxtaps")

SLOPE, OUT_SLOPE = 0.2, 0.1
ONCE_PER_PROCESS = ("RH_CONV_SPLIT_BELOW", "RH_CONV_SPLIT_TARGET", "RH_CONV_NOVEC", "RH_CONV_STAGE_FLOATS")
SHAPES = [(1, 2, 1, 4), (2, 1, 1, 4), (3, 1, 1, 4), (2, 2, 2, 2)]          # conv_params.hpp: rh_conv_f32_by_shape
DMA_VARIANTS = [(True, False), (True, True), (False, True)]                 # (VEC, CTAIL): launch_dma instantiates no (False, False)
LDS_LIMIT = 160 * 1024


def assert_default_planner_env():
    """The planner reads these once per process: a table pinned under one of them describes another planner."""
    for k in ONCE_PER_PROCESS:
        assert k not in os.environ, f"{k} is set: the instance matrix is pinned for the default planner"


def dma_instances():
    return [(s, lk, v) for s in SHAPES for lk in (False, True) for v in DMA_VARIANTS]


def out_len(geo):
    B, Ci, Co, L, k, s, dil, pad, tr = geo[:9]
    if tr:
        return (L - 1) * s - 2 * pad[0] + k
    return (L + pad[0] + pad[1] - dil * (k - 1) - 1) // s + 1


def act_of(row):
    return 2 if "S" in row.ops else (1 if "L" in row.ops else 0)


def desc(L, row):
    """``L`` = rave_amd._lib."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    return L.ConvDesc(batch=B, c_in=Ci, c_out=Co, l_in=Lx, l_out=out_len(row.geo), kernel=k, stride=s, dilation=dil,
                      pad_left=pad[0], transposed=int(tr), groups=1, inner=inner, in_valid=in_valid, act=act_of(row),
                      act_slope=SLOPE, out_act=1 if "o" in row.ops else 0, out_slope=OUT_SLOPE)


def instance_info(L, row, ws=None, align=None):
    """rh_conv1d_f32_instance_info for the call of ``row`` (``ws`` / ``align``: asked for another workspace / alignment)."""
    out = (C.c_int32 * 24)()
    L.check(L.lib.rh_conv1d_f32_instance_info(C.byref(desc(L, row)), row.which, int("b" in row.ops and row.which == 0), int("a" in row.ops),
                                              int((row.align if align is None else align) == 16), int(row.ws if ws is None else ws), out),
            "f32_instance_info")
    v = list(out)
    f = v[6]
    return Info(*(v[:6] + [bool(f & 1), bool(f & 2), bool(f & 4), bool(f & 8)] + v[7:]))


def workspace_bytes(L, row):
    d = desc(L, row)
    fn = L.lib.rh_conv1d_fwd_workspace_bytes if row.which == 0 else L.lib.rh_conv1d_bwd_data_workspace_bytes
    return int(fn(C.byref(d)))


def derive_key(L, row):
    """The Key of the instance the call of ``row`` launches; None = not family 0."""
    assert_default_planner_env()
    i = instance_info(L, row)
    if i.family != 0:
        return None
    if i.ks > 1:
        kmode = "finalize4" if i.finalize == 4 else "finalize"
        assert i.finalize in (1, 4) and row.ws
    else:
        assert i.finalize == 0
        kmode = "nows" if (not row.ws and instance_info(L, row, ws=True).ks > 1) else "unsplit"
    return Key(row.which, i.kernel, i.TM, i.TN, i.WM, i.WN, i.leaky, i.vec, i.ctail, kmode, i.nphase > 1, i.inner > 1)


def _cdiv(a, b):
    return -(-a // b)


def gemm(row):
    """The gather a call is (conv_host.hip: build_plan, rh_conv_fill_fwd / rh_conv_fill_dgrad), restated: GEMM rows M, K channels C,
    columns, strides and the tap offsets of each output phase."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    lo, P = out_len(row.geo), pad[0]

    def phases():
        out = []
        for ph in range(s):
            r0 = (ph + P) % s
            base = (ph + P - r0) // s
            out.append([base - m for m in range(len(range(r0, k, s)))])
        return out

    x_row = in_valid if in_valid else Lx * inner
    if row.which == 0:
        g = dict(C=Ci, M=Co, in_row=x_row, out_row=lo * inner)
        if not tr:
            g.update(offs=[[i * dil - P for i in range(k)]], istr=s, ostr=1, rows=lo)
        else:
            g.update(offs=phases(), istr=1, ostr=s, rows=_cdiv(lo, s))
    else:
        g = dict(C=Co, M=Ci, in_row=lo * inner, out_row=x_row)
        if tr:
            g.update(offs=[[i - P for i in range(k)]], istr=s, ostr=1, rows=Lx)
        elif s == 1:
            g.update(offs=[[P - i * dil for i in range(k)]], istr=1, ostr=1, rows=Lx)
        else:
            g.update(offs=phases(), istr=1, ostr=s, rows=_cdiv(Lx, s))
    g.update(B=B, inner=inner, ncols=g["rows"] * inner, Mp=(g["M"] + 31) & ~31, in_valid=g["in_row"], out_valid=g["out_row"],
             nphase=len(g["offs"]), x_full=Lx * inner)
    return g


def edges(row, i):
    """Names of the tile edges the call of ``row`` sits on (``i`` = its Info)."""
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = row.geo
    g = gemm(row)
    BM = 32 * i.TM * i.WM
    e = set()
    assert (i.nphase, i.inner) == (g["nphase"], inner) and i.gx == _cdiv(B, i.nb) * i.tiles_per_b and i.gy == _cdiv(g["M"], BM), (row, i, g)
    assert i.tiles_per_b == _cdiv(g["ncols"], i.bnl) and i.total_chunks == _cdiv(g["C"], i.ck), (row, i, g)
    if g["ncols"] > i.bnl and g["ncols"] % i.bnl:
        e.add("ragged last column tile")
    if min(B, i.nb) > 1:
        e.add("nb > 1")
        if B > i.nb and B % i.nb:
            e.add("B % nb != 0")
    for name, n in (("ncols == 1", 1), ("ncols == bnl - 1", i.bnl - 1), ("ncols == bnl + 1", i.bnl + 1)):
        if g["ncols"] == n:
            e.add(name)
    if g["M"] < g["Mp"]:
        e.add("M < Mp")
    if g["M"] % BM:
        e.add("partial last row tile")
    if g["C"] % 2:
        e.add("C odd")
    if g["C"] < i.ck:
        e.add("C < ck")
    if i.ck > 2 and g["C"] > i.ck and g["C"] % i.ck == 1:
        e.add("C % ck == 1")
    if i.ck > 2 and g["C"] > i.ck and g["C"] % i.ck == i.ck - 1:
        e.add("C % ck == ck - 1")
    if pad[0] > 0 and pad[1] == 0:
        e.add("causal padding")
    if pad[0] > (k - 1) * dil:
        e.add("padding wider than the left halo")
    if inner > 1 and in_valid and in_valid < Lx * inner:
        e.add("in_valid < in_row")
    if i.kernel == 1:
        if not i.vec and row.align == 16 and inner == 1 and g["in_row"] % 4:
            e.add("in_row % 4 != 0 (VEC off)")
        if i.vec:
            lpr = i.pitch // 4
            for ph in g["offs"]:
                for nt in range(i.tiles_per_b):
                    lo_raw = nt * i.bnl * g["istr"] + min(ph)
                    lo = lo_raw - lo_raw % 4
                    if lo < 0:
                        e.add("VEC boundary tile: lo < 0")
                    if lo + 4 * lpr > g["in_valid"]:
                        e.add("VEC boundary tile: lo + 4 * lpr > in_valid")
            if i.nb * i.ck * (lpr + 1) > 2048:
                e.add("last staged row that fits nx <= 8")
        elif not i.vec and 8 * (((i.maxtaps * i.ck * BM + 255) & ~255) + ((i.nb * i.ck * (i.pitch + 64) + 255) & ~255)) > LDS_LIMIT:
            e.add("last geometry within 160 KiB of LDS")
    if i.lds_fallback:
        e.add("DMA stages beyond 160 KiB of LDS: synchronous kernel")
    return e


EDGES = ["ragged last column tile", "nb > 1", "B % nb != 0", "ncols == 1", "ncols == bnl - 1", "ncols == bnl + 1", "M < Mp",
         "partial last row tile", "C odd", "C < ck", "C % ck == 1", "C % ck == ck - 1", "causal padding", "padding wider than the left halo",
         "in_row % 4 != 0 (VEC off)", "VEC boundary tile: lo < 0", "VEC boundary tile: lo + 4 * lpr > in_valid",
         "last staged row that fits nx <= 8", "VEC refused for its DMA slots", "last geometry within 160 KiB of LDS",
         "DMA stages beyond 160 KiB of LDS: synchronous kernel"]
FINALIZE_OPERANDS = ("bias", "LeakyReLU derivative", "Snake derivative", "add", "output LeakyReLU")


def vec_plan0(row, i):
    """(xrows, lpr) of the VEC attempt of plan_dma (conv_igemm_dma.hip) for a call that is eligible for it, restated; None otherwise.
    The planner reports only the attempt it kept; the rows on the slot / reciprocal bounds are named by the one it dropped."""
    g = gemm(row)
    if g["inner"] != 1 or row.align != 16 or g["in_row"] % 4 or g["C"] >= 192:
        return None
    span = max(max(ph) - min(ph) for ph in g["offs"])
    pitch = ((i.bnl - 1) * g["istr"] + span + 1 + 6) & ~3
    per_ch = i.maxtaps * 32 * i.TM * i.WM + i.nb * pitch
    ck = ((5 * 1024 - 512) // per_ch) & ~1
    if ck < 8:
        ck = ((10 * 1024 - 512) // per_ch) & ~1
    ck = min(max(min(ck, 32), 2), (g["C"] + 1) & ~1)
    return i.nb * ck, pitch // 4


def operands_of(row):
    o = set()
    if row.which == 0:
        o |= {"bias"} if "b" in row.ops else set()
        o |= {"output LeakyReLU"} if "o" in row.ops else set()
    else:
        o |= {"LeakyReLU derivative"} if "L" in row.ops else set()
        o |= {"Snake derivative"} if "S" in row.ops else set()
    return o | ({"add"} if "a" in row.ops else set())


def tags_of(L, row):
    """Every coverage condition of tests/test_f32_matrix_host.py the call of ``row`` meets."""
    key = derive_key(L, row)
    if key is None:
        return set()
    i = instance_info(L, row)
    sh = (i.TM, i.TN, i.WM, i.WN)
    e = edges(row, i)
    p0 = vec_plan0(row, i)
    if i.kernel == 1 and not i.vec and p0 and p0[0] * p0[1] > 2048:
        e.add("VEC refused for its DMA slots")
    t = {("edge", sh, n) for n in e} | {("kmode", sh, key.kmode)}
    if i.kernel == 1 and p0 and p0[0] * p0[1] <= 2048 and (p0[0] * p0[1] - 1) * p0[1] >= 1 << 20:
        t.add(("staged row beyond the exact range of the 20-bit reciprocal",))
    if i.kernel == 1:
        t.add(("dma", sh, i.leaky, (i.vec, i.ctail)))
    else:
        t.add(("sync", sh))
        if row.which == 0 and "S" in row.ops:
            t.add(("sync by a Snake forward", sh))
        if i.lds_fallback:
            t.add(("sync by the LDS fallback",))
    t |= {("finalize", i.finalize, o) for o in operands_of(row)} if i.ks > 1 else set()
    if i.nphase > 1:
        t.add(("phases", i.nphase, "split" if i.ks > 1 else "unsplit"))
    if "in_valid < in_row" in e:
        t.add(("inner", row.which))
        if "nb > 1" in e:
            t.add(("inner, nb > 1",))
    return t


def required():
    """The coverage conditions (tests/test_f32_matrix_host.py asserts each of them on ROWS)."""
    r = [("dma", s, lk, v) for s, lk, v in dma_instances()] + [("sync", s) for s in SHAPES] + [("sync by a Snake forward", s) for s in SHAPES]
    r += [("sync by the LDS fallback",)] + [("kmode", s, km) for s in SHAPES for km in KMODES]
    r += [("finalize", f, o) for f in (1, 4) for o in FINALIZE_OPERANDS]
    r += [("phases", n, m) for n in (2, 3, 4) for m in ("unsplit", "split")]
    r += [("inner", 0), ("inner", 1), ("inner, nb > 1",)] + [("edge", s, e) for s in SHAPES for e in EDGES]
    return r


def seed(name):
    """Python's hash() is salted per process: a plain checksum of the row's name."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def fmt_key(key):
    if key is None:
        return "not family 0"
    return (f"{'fwd' if key.which == 0 else 'dgrad'} {'dma ' if key.kernel else 'sync'} tile={key.TM}{key.TN}{key.WM}{key.WN} "
            f"{'leaky' if key.leaky else 'plain'} {'vec' if key.vec else 'elt'} {'ctail' if key.ctail else 'whole'} {key.kmode:9s} "
            f"{'phases' if key.multiphase else 'single'}{' inner' if key.inner else ''}")


def name_of(which, geo, ops, align, ws):
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = geo
    return (f"{'fwd' if which == 0 else 'dgrad'} {'convT' if tr else 'conv'}{f' s{s}' if s > 1 else ''} {Ci}->{Co} k{k}"
            f"{f' d{dil}' if dil > 1 else ''} B{B} L{Lx} p{pad[0]},{pad[1]}{f' inner{inner}' if inner > 1 else ''}"
            f"{f' valid{in_valid}' if in_valid else ''}{f' [{ops}]' if ops else ''}{' a4' if align == 4 else ''}{'' if ws else ' no-ws'}")


# (which, geo, ops, align, ws, key): the output of `python tests/f32_matrix_search.py cover` (random draws over small geometries,
# the staged-row sweeps of the nx / LDS / 20-bit-reciprocal bounds, then a greedy cover of the conditions of
# tests/test_f32_matrix_host.py, cheapest row first).
_TABLE = [
    (0, (1, 2, 24, 2044, 2, 1, 1916, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 1, 2, 1, 4, False, True, False, 'unsplit', False, False)),
    (0, (1, 2, 24, 2048, 2, 1, 1920, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 24, 10112, 2, 1, 9856, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 24, 10113, 2, 1, 9857, (0, 0), False, 1, 0), 'b', 16, True, (0, 0, 1, 2, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 2, 24, 3020, 2, 1, 2765, (1, 0), False, 1, 0), 'b', 16, True, (0, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 4, 40, 2044, 2, 1, 1916, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 1, 1, 4, False, True, False, 'unsplit', False, False)),
    (0, (1, 4, 40, 2048, 2, 1, 1920, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 40, 10112, 2, 1, 9984, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 40, 10113, 2, 1, 9985, (0, 0), False, 1, 0), 'b', 16, True, (0, 0, 2, 1, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 2, 40, 3148, 2, 1, 2893, (1, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 4, 80, 2044, 2, 1, 1916, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 3, 1, 1, 4, False, True, False, 'unsplit', False, False)),
    (0, (1, 4, 80, 2048, 2, 1, 1920, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 80, 9984, 2, 1, 9856, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 80, 9985, 2, 1, 9857, (0, 0), False, 1, 0), 'b', 16, True, (0, 0, 3, 1, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 2, 80, 3148, 2, 1, 2893, (1, 0), False, 1, 0), 'b', 16, True, (0, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 4, 100, 2044, 2, 1, 1916, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 2, 2, 2, False, True, False, 'unsplit', False, False)),
    (0, (1, 4, 100, 2048, 2, 1, 1920, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 100, 9984, 2, 1, 9856, (0, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (0, (1, 2, 100, 9985, 2, 1, 9857, (0, 0), False, 1, 0), 'b', 16, True, (0, 0, 2, 2, 2, 2, False, False, False, 'unsplit', False, False)),
    (0, (1, 2, 100, 3148, 2, 1, 2893, (1, 0), False, 1, 0), 'b', 16, True, (0, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (1, (1, 3, 3, 2, 2, 1, 9, (11, 0), False, 1, 0), 'La', 16, True, (1, 1, 1, 2, 1, 4, False, True, True, 'unsplit', False, False)),
    (0, (1, 8, 5, 8, 1, 1, 1, (0, 0), True, 1, 0), 'Lb', 16, True, (0, 1, 1, 2, 1, 4, True, True, False, 'unsplit', False, False)),
    (0, (1, 3, 3, 8, 3, 2, 1, (1, 1), False, 1, 0), 'L', 16, True, (0, 1, 1, 2, 1, 4, True, True, True, 'unsplit', False, False)),
    (0, (1, 3, 4, 1, 1, 1, 1, (0, 0), True, 1, 0), 'Lbo', 4, False, (0, 1, 1, 2, 1, 4, True, False, True, 'unsplit', False, False)),
    (1, (1, 33, 3, 8, 1, 1, 1, (0, 0), True, 1, 0), 'La', 16, True, (1, 1, 2, 1, 1, 4, False, True, True, 'unsplit', False, False)),
    (0, (1, 4, 40, 8, 1, 1, 1, (0, 0), True, 1, 0), 'Lbo', 16, True, (0, 1, 2, 1, 1, 4, True, True, False, 'unsplit', False, False)),
    (0, (1, 5, 64, 8, 1, 1, 1, (0, 0), False, 1, 0), 'Lba', 16, True, (0, 1, 2, 1, 1, 4, True, True, True, 'unsplit', False, False)),
    (0, (2, 3, 48, 1, 1, 1, 2, (0, 0), False, 1, 0), 'Lb', 4, True, (0, 1, 2, 1, 1, 4, True, False, True, 'unsplit', False, False)),
    (1, (1, 80, 3, 3, 2, 1, 1, (0, 0), True, 1, 0), 'Sa', 16, True, (1, 1, 3, 1, 1, 4, False, True, True, 'unsplit', False, False)),
    (0, (1, 4, 96, 16, 1, 1, 2, (0, 0), False, 1, 0), 'Lbo', 16, True, (0, 1, 3, 1, 1, 4, True, True, False, 'unsplit', False, False)),
    (0, (1, 5, 96, 8, 1, 1, 1, (0, 0), True, 1, 0), 'L', 16, False, (0, 1, 3, 1, 1, 4, True, True, True, 'unsplit', False, False)),
    (0, (1, 3, 96, 1, 1, 1, 9, (0, 0), False, 1, 0), 'L', 16, False, (0, 1, 3, 1, 1, 4, True, False, True, 'unsplit', False, False)),
    (1, (1, 200, 3, 2, 1, 1, 1, (2, 0), False, 1, 0), 'L', 16, True, (1, 1, 2, 2, 2, 2, False, True, True, 'unsplit', False, False)),
    (0, (1, 4, 200, 8, 1, 1, 1, (0, 0), True, 1, 0), 'L', 16, True, (0, 1, 2, 2, 2, 2, True, True, False, 'unsplit', False, False)),
    (0, (1, 3, 100, 8, 1, 1, 9, (0, 0), False, 1, 0), 'Lba', 16, False, (0, 1, 2, 2, 2, 2, True, True, True, 'unsplit', False, False)),
    (0, (1, 4, 160, 1, 1, 1, 2, (0, 0), False, 1, 0), 'Lbo', 16, True, (0, 1, 2, 2, 2, 2, True, False, True, 'unsplit', False, False)),
    (0, (1, 4, 4, 1, 1, 1, 1, (0, 0), True, 1, 0), 'Sba', 16, True, (0, 0, 1, 2, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 3, 48, 1, 1, 1, 1, (0, 0), True, 1, 0), 'Sb', 16, True, (0, 0, 2, 1, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 15, 80, 1, 1, 1, 2, (0, 0), False, 1, 0), 'S', 4, True, (0, 0, 3, 1, 1, 4, False, False, False, 'unsplit', False, False)),
    (0, (1, 4, 100, 1, 1, 1, 9, (0, 0), False, 1, 0), 'Sb', 4, False, (0, 0, 2, 2, 2, 2, False, False, False, 'unsplit', False, False)),
    (0, (1, 31, 3, 1, 1, 1, 1, (0, 0), False, 1, 0), 'bao', 16, True, (0, 1, 1, 2, 1, 4, False, False, True, 'finalize', False, False)),
    (0, (1, 31, 3, 2, 1, 1, 1, (2, 0), False, 1, 0), 'bao', 16, True, (0, 1, 1, 2, 1, 4, False, False, True, 'finalize4', False, False)),
    (0, (1, 33, 3, 1, 1, 1, 1, (0, 0), True, 1, 0), 'b', 16, False, (0, 1, 1, 2, 1, 4, False, False, True, 'nows', False, False)),
    (1, (1, 48, 48, 1, 1, 1, 9, (0, 0), False, 1, 0), 'L', 4, True, (1, 1, 2, 1, 1, 4, False, False, True, 'finalize', False, False)),
    (0, (1, 40, 48, 2, 2, 1, 2, (4, 0), False, 1, 0), 'bo', 16, True, (0, 1, 2, 1, 1, 4, False, False, True, 'finalize4', False, False)),
    (1, (1, 40, 80, 1, 1, 1, 2, (0, 0), False, 1, 0), 'a', 16, False, (1, 1, 2, 1, 1, 4, False, False, True, 'nows', False, False)),
    (0, (1, 48, 80, 1, 1, 1, 1, (0, 0), False, 1, 0), 'b', 4, True, (0, 1, 3, 1, 1, 4, False, False, True, 'finalize', False, False)),
    (1, (1, 96, 40, 2, 1, 1, 1, (0, 0), False, 2, 0), 'S', 16, True, (1, 1, 3, 1, 1, 4, False, False, True, 'finalize4', False, True)),
    (1, (1, 80, 40, 1, 1, 1, 9, (0, 0), False, 1, 0), '', 4, False, (1, 1, 3, 1, 1, 4, False, False, True, 'nows', False, False)),
    (1, (1, 100, 40, 1, 1, 1, 1, (0, 0), False, 1, 0), 'La', 16, True, (1, 1, 2, 2, 2, 2, False, False, True, 'finalize', False, False)),
    (0, (1, 40, 160, 2, 1, 1, 2, (0, 0), False, 2, 0), 'Lba', 16, True, (0, 1, 2, 2, 2, 2, True, False, True, 'finalize4', False, True)),
    (1, (1, 130, 48, 1, 2, 2, 1, (1, 0), False, 1, 0), 'a', 4, False, (1, 1, 2, 2, 2, 2, False, False, True, 'nows', True, False)),
    (1, (1, 3, 40, 1, 1, 1, 1, (0, 0), True, 1, 0), 'Sa', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'finalize', False, False)),
    (1, (2, 4, 33, 2, 1, 1, 1, (0, 0), False, 2, 0), 'La', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'finalize4', False, True)),
    (1, (1, 3, 32, 2, 2, 2, 1, (1, 0), False, 1, 0), 'S', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'finalize', True, False)),
    (0, (1, 5, 5, 1, 3, 3, 1, (1, 1), True, 1, 0), 'Sb', 4, False, (0, 0, 1, 2, 1, 4, False, False, False, 'unsplit', True, False)),
    (0, (1, 80, 3, 1, 3, 3, 1, (1, 1), True, 1, 0), 'ba', 4, True, (0, 1, 1, 2, 1, 4, False, False, True, 'finalize', True, False)),
    (1, (1, 7, 3, 1, 4, 4, 1, (1, 2), False, 1, 0), '', 4, True, (1, 1, 1, 2, 1, 4, False, False, True, 'unsplit', True, False)),
    (0, (1, 32, 5, 2, 5, 4, 1, (4, 0), True, 1, 0), 'Lbo', 4, True, (0, 1, 1, 2, 1, 4, True, False, True, 'finalize', True, False)),
    (0, (1, 3, 3, 2, 1, 1, 9, (0, 0), False, 5, 6), 'Sba', 4, True, (0, 0, 1, 2, 1, 4, False, False, False, 'unsplit', False, True)),
    (1, (1, 3, 3, 2, 1, 1, 9, (0, 0), False, 2, 3), 'La', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, True)),
    (1, (2, 4, 3, 2, 1, 1, 1, (0, 0), False, 2, 3), 'a', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, True)),
    (1, (1, 3, 3, 257, 1, 1, 9, (0, 0), False, 1, 0), 'L', 4, False, (1, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (5, 3, 3, 33, 1, 1, 9, (2, 0), False, 1, 0), 'Lbo', 16, False, (0, 1, 1, 2, 1, 4, True, False, True, 'unsplit', False, False)),
    (1, (1, 4, 3, 31, 1, 1, 9, (0, 0), False, 1, 0), 'La', 16, True, (1, 1, 1, 2, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (1, 40, 3, 129, 1, 1, 9, (0, 0), False, 1, 0), '', 16, True, (1, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (5, 33, 4, 1, 1, 1, 1, (0, 0), True, 1, 0), 'S', 4, False, (1, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 4, 33, 31, 1, 1, 1, (0, 0), True, 1, 0), 'Sb', 16, True, (0, 0, 2, 1, 1, 4, False, False, False, 'unsplit', False, False)),
    (1, (1, 33, 15, 1, 1, 1, 1, (0, 0), False, 1, 0), 'L', 4, True, (1, 1, 2, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 15, 40, 1, 4, 4, 9, (27, 0), False, 2, 0), 'Lba', 4, False, (0, 1, 2, 1, 1, 4, True, False, True, 'unsplit', False, True)),
    (1, (1, 33, 5, 3, 2, 2, 1, (1, 0), True, 1, 0), 'La', 16, True, (1, 1, 2, 1, 1, 4, False, True, True, 'unsplit', False, False)),
    (1, (1, 80, 3, 129, 1, 1, 1, (0, 0), True, 1, 0), '', 4, True, (1, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (2, 96, 3, 1, 1, 1, 1, (0, 0), False, 1, 0), '', 4, True, (1, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (5, 80, 3, 1, 1, 1, 9, (0, 0), False, 1, 0), '', 16, True, (1, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 3, 80, 31, 1, 1, 1, (0, 0), False, 1, 0), 'a', 4, True, (0, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (1, 80, 17, 1, 3, 1, 2, (2, 2), False, 1, 0), '', 4, True, (1, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (0, (1, 31, 80, 1, 3, 1, 2, (2, 2), False, 1, 0), 'Lba', 4, True, (0, 1, 3, 1, 1, 4, True, False, True, 'finalize', False, False)),
    (1, (1, 96, 3, 1, 1, 1, 2, (2, 0), False, 1, 0), '', 4, True, (1, 1, 3, 1, 1, 4, False, False, True, 'unsplit', False, False)),
    (1, (1, 80, 3, 5, 2, 2, 1, (1, 0), True, 1, 0), 'S', 16, True, (1, 1, 3, 1, 1, 4, False, True, True, 'unsplit', False, False)),
    (1, (1, 100, 3, 129, 1, 1, 1, (0, 0), True, 1, 0), 'La', 16, False, (1, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (1, (2, 100, 3, 1, 1, 1, 1, (0, 0), True, 1, 0), '', 16, False, (1, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (1, (5, 130, 3, 1, 1, 1, 1, (0, 0), True, 1, 0), '', 16, True, (1, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (1, (1, 130, 3, 31, 1, 1, 1, (0, 0), True, 1, 0), 'Sa', 4, False, (1, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (0, (1, 17, 100, 1, 2, 1, 2, (2, 0), False, 1, 0), 'bo', 4, True, (0, 1, 2, 2, 2, 2, False, False, True, 'unsplit', False, False)),
    (0, (1, 15, 130, 1, 2, 1, 2, (2, 0), False, 1, 0), 'Lb', 16, False, (0, 1, 2, 2, 2, 2, True, False, True, 'unsplit', False, False)),
    (0, (1, 3, 100, 8, 2, 1, 2, (2, 0), False, 1, 0), 'L', 16, True, (0, 1, 2, 2, 2, 2, True, True, True, 'unsplit', False, False)),
]
ROWS = [Row(name_of(w, g, o, a, ws), w, g, o, a, ws, None if k is None else Key(*k)) for w, g, o, a, ws, k in _TABLE]
assert len({r.name for r in ROWS}) == len(ROWS)

# Template instances no call can select through the C ABI, with the planner's reason (at most 2 allowed).
UNREACHABLE = []
# Conditions of the kernels' code that no call can reach.
DEAD_CONDITIONS = ["maxtaps > 64 (VEC off): a phase has at most `kernel` taps and conv_host.hip: validate refuses kernel > kMaxTaps = 64"]
