"""The instance matrix of the 1-D weight gradient (csrc/conv_wgrad_x6.hip, csrc/conv_wgrad.hip): one row per direct
``rh_conv1d_bwd_weight_f32`` call, with the kernel instance it must launch (a plain helper module, no fixtures; importing it needs
no GPU).  The counterpart of tests/x6_matrix.py for the forward / data-gradient kernel.

48 x6 instances: ``wgrad_x6_kernel<TM, WM, 4 / WM, AV, PART, PL>`` (40: six (tm, wm) x AV x PART, x PL for tm >= 2) and
``wgrad_x6_wide_kernel<NW, PL>`` (8); the f32-input family adds ``wgrad_dma_kernel<.., RLEAKY, SLEAKY>`` (five tile shapes x three
activation modes x vec / non-vec staging = 30) and ``wgrad_kernel`` (five shapes, snake layers).  ``rh_conv1d_bwd_weight_instance_info``
answers "which one" on the host from route_wgrad1 (conv_wgrad.hip), the function the launch itself goes through.  ``ROWS`` was found by
tests/wgrad_matrix_search.py (a greedy cover over random small geometries); tests/test_wgrad_matrix_host.py proves the coverage from
the diagnostic alone and tests/test_gpu_wgrad_matrix.py runs every row against f64.

Instance key:
  ("x6", tm, wm, AV, PART, PL)     wgrad_x6_kernel<tm, wm, 4 / wm, AV, PART, PL>
  ("wide", NW, PL)                 wgrad_x6_wide_kernel<NW, PL>
  ("dma", bm, bn, leaky, vec)      wgrad_dma_kernel of the bm x bn tile; leaky: 0 none, 1 on R (ConvTranspose1d), 2 on S (Conv1d)
  ("plain", bm, bn)                wgrad_kernel of the bm x bn tile
GEMM view (conv_wgrad_x6.hip): rows m < M, columns (c, t) < N = C T, reduction over B x r_row positions of R; Conv1d: R = dy
(M = c_out, r_row = l_out), S = x; ConvTranspose1d: R = x (M = c_in, r_row = l_in), S = dy.
"""
import ctypes as C
import os
from collections import namedtuple

# geo = (B, Cin, Cout, L, k, stride, dilation, (pad_left, pad_right), transposed); L = length of the conv's INPUT x
# act = "" | "L" LeakyReLU(0.2) on the conv's input | "S" snake on the conv's input
# bias = a bias gradient is asked for; off = byte offset of the dy and x pointers from 16-byte alignment (0 or 4)
# env = the RH_WGRAD_X6* switches of the call, ((name, value), ...); armed = both range slots are armed
Row = namedtuple("Row", "name geo act bias off env armed key")

SLOPE = 0.2
PER_CALL = ("RH_WGRAD_X6", "RH_WGRAD_X6_PLANES", "RH_WGRAD_X6_WIDE", "RH_WGRAD_X6_BLOCKS")
ONCE_PER_PROCESS = ("RH_WGRAD_X6_TM", "RH_WGRAD_X6_ALL", "RH_WGRAD_RK", "RH_WGRAD_RK_INNER", "RH_WGRAD_BLOCKS", "RH_WGRAD_MINCHUNKS",
                    "RH_WGRAD_NOVEC")
KINDS = ("4-wave", "4-wave PL", "wide", "wide PL", "dma vec", "dma non-vec")
F0_SHAPES = ((32, 256), (64, 128), (96, 96), (96, 128), (128, 128))        # conv_wgrad.hip: w_shape, and the ladder in route_wgrad1


class Env:
    """Sets the given variables for the duration; a value of None removes the variable."""

    def __init__(self, kv):
        self.kv = dict(kv)

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


def assert_default_planner_env():
    """The planner reads these once per process: a table pinned under one of them describes another planner."""
    for k in ONCE_PER_PROCESS:
        assert k not in os.environ, f"{k} is set: the instance matrix is pinned for the default planner"


def call_env(row, **more):
    """The four per-call switches for a call of ``row``: unset unless the row (or ``more``) sets them."""
    kv = {k: None for k in PER_CALL}
    kv.update(dict(row.env))
    kv.update(more)
    return Env(kv)


def x6_instances():
    out = [("x6", tm, wm, av, part, pl) for tm, wm in ((1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (3, 2)) for av in (0, 1) for part in (0, 1)
           for pl in ((0, 1) if tm >= 2 else (0,))]
    return out + [("wide", nw, pl) for nw in (3, 4, 6, 9) for pl in (0, 1)]


def f0_instances():
    return ([("dma", bm, bn, lk, vec) for bm, bn in F0_SHAPES for lk in (0, 1, 2) for vec in (0, 1)]
            + [("plain", bm, bn) for bm, bn in F0_SHAPES])


def out_len(geo):
    B, Ci, Co, L, k, s, dil, pad, tr = geo
    if tr:
        return (L - 1) * s - 2 * pad[0] + k
    return (L + pad[0] + pad[1] - dil * (k - 1) - 1) // s + 1


def gemm(geo):
    """The GEMM of the call (conv_wgrad.hip: fill), restated: M rows, C channels x T taps of columns, r_row positions of R per batch
    item, s_row of S, the stride between positions in S and the tap offsets."""
    B, Ci, Co, L, k, s, dil, pad, tr = geo
    if tr:
        off = [t - pad[0] for t in range(k)]
        return dict(M=Ci, C=Co, T=k, N=Co * k, r_row=L, s_row=out_len(geo), istride=s, off=off)
    off = [t * dil - pad[0] for t in range(k)]
    return dict(M=Co, C=Ci, T=k, N=Ci * k, r_row=out_len(geo), s_row=L, istride=s, off=off)


def desc(L, row):
    """``L`` = rave_amd._lib."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    return L.ConvDesc(batch=B, c_in=Ci, c_out=Co, l_in=Lx, l_out=out_len(row.geo), kernel=k, stride=s, dilation=dil, pad_left=pad[0],
                      transposed=int(tr), groups=1, inner=1, in_valid=0, act={"": 0, "L": 1, "S": 2}[row.act], act_slope=SLOPE,
                      out_act=0, out_slope=0.0)


def instance_info(L, row, **more):
    """The 16 numbers of rh_conv1d_bwd_weight_instance_info for the call of ``row`` (under the row's switches, plus ``more``)."""
    out = (C.c_int32 * 16)()
    with call_env(row, **more):
        L.check(L.lib.rh_conv1d_bwd_weight_instance_info(C.byref(desc(L, row)), int(row.off == 0), int(row.off == 0), int(row.armed), out),
                "instance_info")
    return tuple(out)


def workspace_bytes(L, row, **more):
    with call_env(row, **more):
        return int(L.lib.rh_conv1d_workspace_bytes(C.byref(desc(L, row))))


def key_of(info):
    if info[0] == 1:
        return ("wide", info[2], info[6]) if info[1] else ("x6", info[2], info[3], info[4], info[5], info[6])
    if info[0] == 0:
        return ("dma", info[1], info[2], info[5], info[4]) if info[3] else ("plain", info[1], info[2])
    return ("family", info[0])


def kind_of(info):
    """Which of KINDS the launch is (None: wgrad_kernel, another family)."""
    if info[0] == 1:
        return ("wide" if info[1] else "4-wave") + (" PL" if info[6] else "")
    if info[0] == 0 and info[3]:
        return "dma vec" if info[4] else "dma non-vec"
    return None


def slicing(info):
    """(Z, K units per slice, K units in all, K units per batch item, positions per unit, tile rows, tile columns) of either family;
    a K unit is a 32-position step (family 1) or an rk-position chunk (family 0)."""
    if info[0] == 1:
        return dict(Z=info[7], per_z=info[8], total=info[9], per_b=info[12], span=32, rows=info[10], cols=info[11])
    return dict(Z=info[7], per_z=info[8], total=info[9], per_b=info[10], span=info[6], rows=info[1], cols=info[2])


def edges(row, info):
    """Names of the edges of the staging / tile addressing this call sits on, from the diagnostic's numbers and the geometry."""
    B, Ci, Co, Lx, k, s, dil, pad, tr = row.geo
    g, sl = gemm(row.geo), slicing(info)
    e = set()
    r_row, M, N, T = g["r_row"], g["M"], g["N"], g["T"]
    if r_row % 32 and r_row % 4 == 0:
        e.add("r_row % 32 != 0, r_row % 4 == 0")
    if r_row % 4:
        e.add("r_row % 4 != 0")
    if r_row < 32:
        e.add("r_row < 32")
    if not tr and k > 1:
        e.add({(0, 0): "no pad", (1, 0): "left pad only", (0, 1): "right pad only", (1, 1): "both pads"}[(int(pad[0] > 0), int(pad[1] > 0))])
        if s == 1 and dil in (1, 9):
            e.add(f"dilation {dil}")
    reach = max(g["off"]) - min(g["off"])
    if info[0] == 1 and s == 1 and T >= 2 and (32 + reach + 7) // 8 > 7 and (dict(row.env).get("RH_WGRAD_X6_PLANES") == 1 or info[1]):
        assert not info[6]
        e.add("reach beyond the plane image")
    if M % 32:
        e.add("M % 32 != 0")
    if M % sl["rows"]:
        e.add("partial last row tile")
        if info[0] == 1 and not info[1] and info[3] == 2:
            e.add("partial last row tile at wm == 2")
    if T == 3 and N > sl["cols"] and sl["cols"] % T:
        e.add("tile starts mid-channel")
    if info[0] == 1 and not info[1] and info[5]:
        # PART: live_tn of the waves of the last workgroup column tile (the others are full: 2)
        wn_count, n0 = 4 // info[3], (-(-N // sl["cols"]) - 1) * sl["cols"]
        live = {2} if n0 > 0 else set()
        for wn in range(wn_count):
            live.add(0 if n0 + 64 * wn >= N else (1 if n0 + 64 * wn + 32 >= N else 2))
        if live == {0, 1, 2}:
            e.add("live_tn 0, 1 and 2")
    if sl["Z"] == 1:
        e.add("Z == 1")
    else:
        e.add("Z > 1")
        if sl["total"] % sl["per_z"]:
            e.add("short last K slice")
        if sl["per_b"] % sl["per_z"]:
            e.add("K slice crosses a batch item")
    if s > 1:
        e.add(f"{'ConvTranspose1d' if tr else 'Conv1d'} stride {s}")
    fused = info[0] == 1 and not tr
    e.add(("bias" if row.bias else "no bias") + (", Z == 1" if sl["Z"] == 1 else ", Z > 1"))
    if row.bias:
        e.add("fused bias row sums" if fused else "bias through rh_bias_grad_launch")
    return e


ALWAYS = ["r_row % 32 != 0, r_row % 4 == 0", "r_row % 4 != 0", "r_row < 32", "no pad", "left pad only", "right pad only", "both pads",
          "dilation 1", "dilation 9", "M % 32 != 0", "partial last row tile", "Z == 1", "short last K slice", "K slice crosses a batch item",
          "bias, Z == 1", "bias, Z > 1", "no bias, Z == 1", "no bias, Z > 1"]
STRIDED = ["Conv1d stride 2", "Conv1d stride 4", "ConvTranspose1d stride 2", "ConvTranspose1d stride 4"]
REQUIRED = {
    "4-wave": ALWAYS + STRIDED + ["reach beyond the plane image", "partial last row tile at wm == 2", "tile starts mid-channel",
                                  "live_tn 0, 1 and 2", "fused bias row sums", "bias through rh_bias_grad_launch"],
    "4-wave PL": ALWAYS + ["partial last row tile at wm == 2", "tile starts mid-channel", "live_tn 0, 1 and 2", "fused bias row sums"],
    "wide": ALWAYS + STRIDED + ["reach beyond the plane image", "fused bias row sums", "bias through rh_bias_grad_launch"],
    "wide PL": ALWAYS + ["fused bias row sums"],
    "dma vec": ALWAYS + STRIDED + ["tile starts mid-channel", "bias through rh_bias_grad_launch"],
    "dma non-vec": ALWAYS + STRIDED + ["tile starts mid-channel", "bias through rh_bias_grad_launch"],
}
# (kind, edge) pairs of REQUIRED that do not exist, with the reason
NOT_APPLICABLE = {
    ("dma vec", "r_row % 4 != 0"): "the 16-byte DMA staging needs r_row % 4 == 0 (conv_wgrad.hip: w_configure)",
    ("wide", "dilation 1"): "a stride-1 layer with several taps and reach <= 24 always takes plane staging on the wide tile",
    ("wide", "dilation 9"): "a stride-1 layer with several taps and reach <= 24 always takes plane staging on the wide tile",
}


def seed(name):
    """Python's hash() is salted per process: a plain checksum of the row's name."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def fmt_key(key):
    if key[0] == "x6":
        return f"wgrad_x6_kernel<{key[1]}, {key[2]}, {4 // key[2]}, AV={key[3]}, PART={key[4]}, PL={key[5]}>"
    if key[0] == "wide":
        return f"wgrad_x6_wide_kernel<{key[1]}, PL={key[2]}>"
    if key[0] == "dma":
        return f"wgrad_dma_kernel {key[1]}x{key[2]} leaky={('none', 'R', 'S')[key[3]]} vec={key[4]}"
    if key[0] == "plain":
        return f"wgrad_kernel {key[1]}x{key[2]}"
    return f"family {key[1]}"


def make_name(geo, act, bias, off, env, armed):
    B, Ci, Co, Lx, k, s, dil, pad, tr = geo
    sw = " ".join(f"{n[len('RH_WGRAD_'):]}={v}" for n, v in env)
    return (f"{'convT' if tr else 'conv'}{f' s{s}' if s > 1 else ''} {Ci}->{Co} k{k}{f' d{dil}' if dil > 1 else ''} B{B} L{Lx} p{pad[0]},{pad[1]}"
            f"{f' [{act}]' if act else ''}{' +b' if bias else ''}{f' off{off}' if off else ''}{f' {sw}' if sw else ''}{'' if armed else ' unarmed'}")


# (geo, act, bias, off, env, armed, key): printed by tests/wgrad_matrix_search.py
_X6, _PLANES, _WIDE, _BLOCKS = PER_CALL
_TABLE = [
    ((5, 32, 10, 224, 2, 2, 1, (0, 0), True), '', False, 4, ((_BLOCKS, 2),), True, ('dma', 32, 256, 0, 0)),
    ((5, 8, 32, 224, 3, 1, 9, (18, 0), False), '', True, 0, ((_WIDE, 0),), True, ('dma', 32, 256, 0, 1)),
    ((1, 32, 8, 20, 4, 4, 1, (0, 0), True), 'L', False, 4, ((_BLOCKS, 1),), True, ('dma', 32, 256, 1, 0)),
    ((5, 32, 8, 300, 2, 2, 1, (0, 0), True), 'L', False, 0, ((_BLOCKS, 2),), True, ('dma', 32, 256, 1, 1)),
    ((5, 8, 32, 300, 3, 1, 9, (0, 18), False), 'L', True, 4, ((_WIDE, 0),), True, ('dma', 32, 256, 2, 0)),
    ((1, 8, 32, 32, 4, 4, 1, (0, 3), False), 'L', False, 0, ((_WIDE, 0),), True, ('dma', 32, 256, 2, 1)),
    ((1, 43, 40, 20, 3, 1, 1, (0, 0), False), '', True, 0, ((_X6, 0),), True, ('dma', 64, 128, 0, 0)),
    ((1, 10, 40, 32, 2, 2, 1, (0, 0), False), '', False, 0, ((_X6, 0),), True, ('dma', 64, 128, 0, 1)),
    ((1, 40, 8, 20, 2, 2, 1, (0, 0), True), 'L', True, 4, ((_BLOCKS, 1),), True, ('dma', 64, 128, 1, 0)),
    ((1, 40, 8, 20, 4, 4, 1, (0, 0), True), 'L', True, 0, ((_X6, 0),), True, ('dma', 64, 128, 1, 1)),
    ((1, 10, 40, 20, 2, 2, 1, (1, 0), False), 'L', False, 0, ((_PLANES, 1),), True, ('dma', 64, 128, 2, 0)),
    ((1, 43, 40, 28, 3, 1, 1, (1, 1), False), 'L', True, 0, ((_X6, 0),), True, ('dma', 64, 128, 2, 1)),
    ((1, 32, 70, 20, 3, 1, 1, (0, 0), False), '', True, 0, ((_X6, 0),), True, ('dma', 96, 96, 0, 0)),
    ((1, 32, 70, 20, 3, 1, 1, (0, 2), False), '', True, 0, ((_X6, 0),), True, ('dma', 96, 96, 0, 1)),
    ((1, 96, 48, 20, 2, 2, 1, (0, 0), True), 'L', False, 4, ((_X6, 0),), True, ('dma', 96, 96, 1, 0)),
    ((1, 70, 24, 20, 4, 4, 1, (0, 0), True), 'L', True, 0, ((_X6, 0),), True, ('dma', 96, 96, 1, 1)),
    ((1, 96, 70, 20, 1, 1, 1, (0, 0), False), 'L', False, 4, ((_X6, 0),), True, ('dma', 96, 96, 2, 0)),
    ((1, 96, 70, 20, 1, 1, 1, (0, 0), False), 'L', True, 0, ((_X6, 0),), True, ('dma', 96, 96, 2, 1)),
    ((1, 8, 80, 20, 4, 4, 1, (1, 2), False), '', True, 0, ((_X6, 0),), True, ('dma', 96, 128, 0, 0)),
    ((1, 8, 80, 20, 1, 1, 1, (0, 0), False), '', True, 0, (), True, ('dma', 96, 128, 0, 1)),
    ((1, 70, 8, 20, 2, 2, 1, (0, 0), True), 'L', True, 4, ((_PLANES, 1), (_BLOCKS, 1)), True, ('dma', 96, 128, 1, 0)),
    ((1, 70, 10, 20, 2, 2, 1, (0, 0), True), 'L', True, 0, ((_BLOCKS, 2),), True, ('dma', 96, 128, 1, 1)),
    ((1, 8, 70, 31, 1, 1, 1, (0, 0), False), 'L', True, 4, ((_PLANES, 1), (_BLOCKS, 1)), True, ('dma', 96, 128, 2, 0)),
    ((1, 8, 70, 20, 1, 1, 1, (0, 0), False), 'L', True, 0, ((_WIDE, 0),), True, ('dma', 96, 128, 2, 1)),
    ((1, 8, 100, 31, 1, 1, 1, (0, 0), False), '', True, 0, (), True, ('dma', 128, 128, 0, 0)),
    ((1, 8, 100, 20, 1, 1, 1, (0, 0), False), '', False, 0, (), True, ('dma', 128, 128, 0, 1)),
    ((1, 128, 8, 20, 2, 2, 1, (0, 0), True), 'L', False, 4, ((_PLANES, 1),), True, ('dma', 128, 128, 1, 0)),
    ((1, 200, 8, 20, 2, 2, 1, (0, 0), True), 'L', False, 0, ((_BLOCKS, 2),), True, ('dma', 128, 128, 1, 1)),
    ((1, 10, 100, 20, 1, 1, 1, (0, 0), False), 'L', True, 4, (), True, ('dma', 128, 128, 2, 0)),
    ((1, 8, 100, 28, 1, 1, 1, (0, 0), False), 'L', True, 0, ((_WIDE, 0),), True, ('dma', 128, 128, 2, 1)),
    ((1, 8, 32, 20, 3, 1, 9, (0, 18), False), 'S', False, 0, ((_PLANES, 1), (_BLOCKS, 1)), True, ('plain', 32, 256)),
    ((1, 8, 64, 20, 1, 1, 1, (0, 0), False), 'S', False, 0, ((_PLANES, 1),), True, ('plain', 64, 128)),
    ((1, 32, 80, 20, 3, 1, 9, (0, 0), False), 'S', False, 0, (), True, ('plain', 96, 96)),
    ((1, 8, 70, 20, 1, 1, 1, (0, 0), False), 'S', False, 0, ((_BLOCKS, 1),), True, ('plain', 96, 128)),
    ((1, 8, 256, 20, 1, 1, 1, (0, 0), False), 'S', False, 4, (), True, ('plain', 128, 128)),
    ((1, 43, 70, 20, 2, 2, 1, (1, 0), False), 'L', True, 0, ((_BLOCKS, 1),), True, ('wide', 3, 0)),
    ((1, 43, 70, 20, 2, 2, 1, (0, 0), False), 'L', False, 0, (), True, ('wide', 3, 0)),
    ((1, 70, 22, 20, 4, 4, 1, (0, 0), True), '', True, 0, (), True, ('wide', 3, 0)),
    ((1, 32, 70, 20, 3, 1, 1, (0, 0), False), '', True, 4, ((_BLOCKS, 2),), True, ('wide', 3, 1)),
    ((3, 70, 54, 70, 2, 2, 1, (0, 0), True), '', True, 0, (), True, ('wide', 4, 0)),
    ((1, 16, 80, 28, 7, 1, 1, (6, 0), False), '', False, 4, (), True, ('wide', 4, 1)),
    ((1, 54, 70, 28, 3, 1, 13, (13, 13), False), 'L', False, 0, (), True, ('wide', 6, 0)),
    ((3, 43, 70, 70, 3, 1, 9, (0, 18), False), 'L', True, 0, (), True, ('wide', 6, 1)),
    ((5, 32, 80, 150, 8, 4, 1, (0, 7), False), '', False, 4, (), True, ('wide', 9, 0)),
    ((2, 80, 80, 100, 3, 1, 1, (1, 1), False), 'L', False, 4, ((_BLOCKS, 2),), True, ('wide', 9, 1)),
    ((1, 80, 32, 20, 3, 1, 9, (0, 0), False), '', False, 4, ((_PLANES, 1), (_BLOCKS, 1)), True, ('x6', 1, 1, 0, 0, 0)),
    ((3, 32, 16, 70, 4, 2, 1, (0, 0), True), '', True, 4, (), True, ('x6', 1, 1, 0, 1, 0)),
    ((1, 80, 32, 20, 3, 1, 9, (0, 18), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 1, 1, 1, 0, 0)),
    ((3, 22, 32, 100, 3, 1, 9, (0, 18), False), 'L', False, 0, ((_PLANES, 0),), True, ('x6', 1, 1, 1, 1, 0)),
    ((1, 144, 54, 20, 2, 2, 1, (0, 0), True), 'L', False, 4, ((_BLOCKS, 1),), True, ('x6', 1, 2, 0, 0, 0)),
    ((1, 32, 144, 20, 2, 2, 1, (0, 1), False), '', False, 4, ((_PLANES, 1),), True, ('x6', 1, 2, 0, 1, 0)),
    ((1, 16, 144, 20, 7, 1, 1, (3, 3), False), '', False, 0, ((_PLANES, 0),), True, ('x6', 1, 2, 1, 0, 0)),
    ((1, 64, 144, 20, 1, 1, 1, (0, 0), False), 'L', False, 0, ((_PLANES, 0),), True, ('x6', 1, 2, 1, 1, 0)),
    ((1, 64, 40, 20, 4, 2, 1, (3, 0), False), 'L', True, 4, ((_BLOCKS, 2),), True, ('x6', 2, 1, 0, 0, 0)),
    ((1, 80, 40, 20, 3, 1, 1, (0, 0), False), 'L', True, 0, (), True, ('x6', 2, 1, 0, 0, 1)),
    ((1, 8, 40, 20, 8, 4, 1, (7, 0), False), '', False, 4, ((_PLANES, 0),), True, ('x6', 2, 1, 0, 1, 0)),
    ((3, 22, 40, 70, 3, 1, 9, (9, 9), False), 'L', True, 0, (), True, ('x6', 2, 1, 0, 1, 1)),
    ((1, 80, 40, 28, 3, 1, 13, (0, 26), False), '', True, 0, ((_WIDE, 0),), True, ('x6', 2, 1, 1, 0, 0)),
    ((1, 80, 40, 20, 3, 1, 9, (18, 0), False), 'L', True, 0, ((_BLOCKS, 2),), True, ('x6', 2, 1, 1, 0, 1)),
    ((1, 32, 40, 32, 2, 2, 1, (0, 0), False), 'L', False, 0, ((_PLANES, 0),), True, ('x6', 2, 1, 1, 1, 0)),
    ((1, 10, 40, 20, 7, 1, 1, (0, 6), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 2, 1, 1, 1, 1)),
    ((1, 16, 100, 20, 7, 1, 1, (3, 3), False), '', False, 4, ((_PLANES, 0),), True, ('x6', 2, 2, 0, 0, 0)),
    ((1, 80, 100, 20, 3, 1, 9, (9, 9), False), 'L', False, 4, ((_PLANES, 1),), True, ('x6', 2, 2, 0, 0, 1)),
    ((1, 32, 100, 20, 2, 2, 1, (0, 1), False), '', False, 0, (), True, ('x6', 2, 2, 0, 1, 0)),
    ((1, 22, 128, 20, 3, 1, 1, (2, 0), False), 'L', False, 4, ((_PLANES, 1), (_BLOCKS, 1)), True, ('x6', 2, 2, 0, 1, 1)),
    ((1, 100, 54, 20, 2, 2, 1, (0, 0), True), '', True, 0, ((_PLANES, 0),), True, ('x6', 2, 2, 1, 0, 0)),
    ((1, 16, 128, 28, 7, 1, 1, (6, 0), False), 'L', True, 0, ((_PLANES, 1),), True, ('x6', 2, 2, 1, 0, 1)),
    ((1, 43, 100, 20, 3, 1, 1, (1, 1), False), '', True, 0, (), True, ('x6', 2, 2, 1, 1, 0)),
    ((1, 43, 100, 20, 3, 1, 1, (2, 0), False), 'L', True, 0, ((_PLANES, 1),), True, ('x6', 2, 2, 1, 1, 1)),
    ((1, 80, 70, 20, 3, 1, 1, (0, 0), False), '', False, 0, ((_PLANES, 0),), True, ('x6', 3, 1, 0, 0, 0)),
    ((1, 80, 80, 20, 3, 1, 1, (0, 0), False), 'L', False, 4, ((_WIDE, 0),), True, ('x6', 3, 1, 0, 0, 1)),
    ((1, 70, 16, 20, 4, 4, 1, (0, 0), True), 'L', False, 4, ((_PLANES, 1),), True, ('x6', 3, 1, 0, 1, 0)),
    ((1, 22, 70, 20, 3, 1, 1, (0, 0), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 3, 1, 0, 1, 1)),
    ((1, 80, 70, 20, 3, 1, 1, (1, 1), False), 'L', True, 0, ((_PLANES, 0),), True, ('x6', 3, 1, 1, 0, 0)),
    ((1, 80, 70, 20, 3, 1, 9, (9, 9), False), 'L', True, 0, ((_WIDE, 0),), True, ('x6', 3, 1, 1, 0, 1)),
    ((1, 24, 70, 28, 3, 1, 13, (26, 0), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 3, 1, 1, 1, 0)),
    ((3, 22, 80, 70, 3, 1, 1, (0, 0), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 3, 1, 1, 1, 1)),
    ((1, 16, 192, 20, 7, 1, 1, (0, 0), False), '', False, 0, ((_PLANES, 0),), True, ('x6', 3, 2, 0, 0, 0)),
    ((1, 80, 192, 20, 3, 1, 9, (9, 9), False), 'L', False, 4, ((_PLANES, 1), (_BLOCKS, 1)), True, ('x6', 3, 2, 0, 0, 1)),
    ((1, 32, 192, 20, 2, 2, 1, (0, 1), False), 'L', True, 4, ((_PLANES, 1),), True, ('x6', 3, 2, 0, 1, 0)),
    ((1, 22, 192, 20, 3, 1, 1, (0, 0), False), 'L', False, 0, ((_PLANES, 1),), True, ('x6', 3, 2, 0, 1, 1)),
    ((1, 192, 54, 20, 2, 2, 1, (0, 0), True), 'L', False, 0, ((_BLOCKS, 1),), True, ('x6', 3, 2, 1, 0, 0)),
    ((1, 16, 192, 20, 7, 1, 1, (3, 3), False), '', False, 0, ((_PLANES, 1),), True, ('x6', 3, 2, 1, 0, 1)),
    ((1, 192, 32, 20, 2, 2, 1, (0, 0), True), 'L', True, 0, ((_PLANES, 0),), True, ('x6', 3, 2, 1, 1, 0)),
    ((1, 22, 192, 20, 3, 1, 9, (9, 9), False), 'L', True, 0, ((_PLANES, 1), (_BLOCKS, 1)), True, ('x6', 3, 2, 1, 1, 1)),
    # the silent fallback: x6-eligible geometries (their armed twins are rows above) WITHOUT range slots take the f32-input kernels
    ((2, 80, 80, 100, 3, 1, 1, (1, 1), False), 'L', True, 0, (), False, ('dma', 96, 128, 2, 1)),
    ((1, 43, 100, 20, 3, 1, 1, (1, 1), False), '', True, 0, (), False, ('dma', 128, 128, 0, 1)),
]
ROWS = [Row(make_name(g, a, b, o, e, r), g, a, b, o, e, r, k) for g, a, b, o, e, r, k in _TABLE]
assert len({r.name for r in ROWS}) == len(ROWS)

# instances no call can select through the C ABI under the default planner, with the reason: (key, reason)
UNREACHABLE = []
