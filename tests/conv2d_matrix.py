"""The instance matrix of the 2-D convolution kernels (csrc/conv2d.hip, conv2d_x6.hip, wgrad2d_x6.hip, conv2d_smallm.hip,
conv2d_smallc.hip): one row per direct ``rh_conv2d_fwd_f32`` / ``rh_conv2d_bwd_data_f32`` / ``rh_conv2d_bwd_weight_f32`` call, with the
kernel instance it must launch (a plain helper module, no fixtures; importing it needs no GPU).  The 2-D counterpart of
tests/x6_matrix.py and tests/wgrad_matrix.py.

``rh_conv2d_instance_info`` answers "which one" on the host from the selection and planning code the launch itself runs.  ``ROWS`` was
found by tests/conv2d_matrix_search.py (a greedy cover over random small geometries); tests/test_conv2d_matrix_host.py proves the
coverage from the diagnostic alone and tests/test_gpu_conv2d_matrix.py runs every row against f64.

Instance key (which: 0 forward, 1 data gradient):
  ("x6", which, TM, TN, NQ)            conv2d_x6_kernel<TM, TN, NQ>
  ("dma", which, TM, TN, WM, WN)       conv2d_dma_kernel<TM, TN, WM, WN>
  ("igemm", which, TM, TN, WM, WN)     conv2d_igemm_kernel<TM, TN, WM, WN>
  ("smallm", KH, MM, FLIP)             conv2d_smallm_kernel<KH, MM, FLIP>   (FLIP = 1: data gradient)
  ("smallc", KH)                       conv2d_smallc_fwd_kernel<KH>
  ("wx6", NQX, SW)                     wgrad2d_x6_kernel<NQX, SW>
  ("wdma", TN)                         wgrad2d_dma_kernel<TN>
  ("wgrad", TM, TN, WM, WN)            wgrad2d_kernel<TM, TN, WM, WN>
"""
import ctypes as C
import os
from collections import namedtuple

# which = 0 forward, 1 data gradient, 2 weight gradient
# geo = (B, Cin, Cout, H, W, (kh, kw), (sh, sw), (dh, dw), (ph, pw)); H x W = the plane of the conv's INPUT x
# act = "" | "L": forward: LeakyReLU(SLOPE) on the output; backward calls: the FUSED derivative (act = LEAKY in the descriptor, y given)
# bias = forward: a bias is added; weight gradient: a bias gradient is asked for
# off = byte offset of the activation pointers from 16-byte alignment (0 or 4); the packed operand stays aligned
# env = the per-call switches of the call, ((name, value), ...); armed = the range slots are armed
# ws = weight gradient: True: rh_conv2d_workspace_bytes is offered; False: only what the f32-input launch needs (withheld)
Row = namedtuple("Row", "name which geo act bias off env armed ws key")

SLOPE = 0.2
PER_CALL = ("RH_CONV2D_X6", "RH_CONV2D_SMALLM", "RH_CONV_X6", "RH_WGRAD2D_X6")
ONCE_PER_PROCESS = ("RH_CONV2D_X6_TN", "RH_CONV2D_STAGE_FLOATS", "RH_CONV2D_DMA_STAGE_FLOATS", "RH_WGRAD2D_DMA_STAGE_FLOATS",
                    "RH_WGRAD2D_LDS_BYTES", "RH_WGRAD2D_X6_SLICES", "RH_CONV2D_NODMA", "RH_WGRAD2D_NODMA")
KERNELS = ("x6", "dma", "igemm", "smallm", "smallc", "wx6", "wdma", "wgrad")       # rh_conv2d_instance_info: out[0]
F0_TILES = ((1, 2, 1, 4), (2, 1, 1, 4), (3, 1, 1, 4), (2, 2, 2, 2))                # conv2d_f32.hip: tile2_of
X6_TILES = ((1, 2, 4), (1, 2, 8), (1, 1, 4), (1, 1, 8), (2, 2, 4), (2, 2, 8), (2, 1, 4), (2, 1, 8), (3, 1, 4), (3, 1, 8))
MAX_B, MAX_CH, MAX_NUMEL = 5, 160, 1 << 19


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
    """The planners read these once per process: a table pinned under one of them describes another planner.  RH_WGRAD_X6 (the switch
    of the 1-D weight gradient, which also turns wgrad2d_x6_kernel off) is read per call, but no row sets it: it must be unset too."""
    for k in ONCE_PER_PROCESS + ("RH_WGRAD_X6",):
        assert k not in os.environ, f"{k} is set: the instance matrix is pinned for the default planner"


def call_env(row, **more):
    """The per-call switches for a call of ``row``: unset unless the row (or ``more``) sets them."""
    kv = {k: None for k in PER_CALL}
    kv.update(dict(row.env))
    kv.update(more)
    return Env(kv)


def instances():
    """Every instance the product build compiles, from the tables above: conv2d_x6.hip's RH_C2X_CASE list, the four family-0 tiles
    (each as DMA and register-staged kernel, forward and data gradient, and as wgrad2d_kernel), and the switches of
    rh_wgrad2d_x6_launch, run_w2, rh_conv2d_smallm_launch and rh_conv2d_smallc_fwd_launch."""
    out = [("x6", w) + t for t in X6_TILES for w in (0, 1)]
    out += [(k, w) + t for k in ("dma", "igemm") for t in F0_TILES for w in (0, 1)]
    out += [("wgrad",) + t for t in F0_TILES]
    out += [("wdma", tn) for tn in (1, 2, 4)]
    out += [("wx6", 3, 1), ("wx6", 6, 1), ("wx6", 3, 2)]
    out += [("smallm", kh, mm, flip) for kh in (3, 9) for mm in (1, 2, 4) for flip in (0, 1)]
    out += [("smallc", 3), ("smallc", 9)]
    return out


def out_hw(geo):
    B, Ci, Co, H, W, k, s, dil, pad = geo
    return ((H + 2 * pad[0] - dil[0] * (k[0] - 1) - 1) // s[0] + 1, (W + 2 * pad[1] - dil[1] * (k[1] - 1) - 1) // s[1] + 1)


def valid(geo):
    B, Ci, Co, H, W, k, s, dil, pad = geo
    return (H + 2 * pad[0] - dil[0] * (k[0] - 1) - 1 >= 0 and W + 2 * pad[1] - dil[1] * (k[1] - 1) - 1 >= 0 and k[0] * k[1] <= 64
            and s[0] * s[1] <= 8)


def numels(geo):
    B, Ci, Co, H, W, k, s, dil, pad = geo
    ho, wo = out_hw(geo)
    return (B * Ci * H * W, B * Co * ho * wo, Co * Ci * k[0] * k[1])


def desc(L, row):
    """``L`` = rave_amd._lib.  A forward call carries its output activation; a backward call carries one only on the fused-derivative
    rows (rave_amd.ops folds act'(y) into dy and passes NONE)."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    ho, wo = out_hw(row.geo)
    return L.Conv2dDesc(batch=B, c_in=Ci, c_out=Co, h_in=H, w_in=W, h_out=ho, w_out=wo, kh=k[0], kw=k[1], sh=s[0], sw=s[1], dh=dil[0],
                        dw=dil[1], ph=pad[0], pw=pad[1], act=1 if row.act == "L" else 0, act_slope=SLOPE)


def workspace_bytes(L, row):
    """The bytes the call of ``row`` offers: rh_conv2d_workspace_bytes, or (withheld) the bias scratch plus what the f32-input launch
    of the same call needs."""
    if row.which != 2:
        return 0
    full = int(L.lib.rh_conv2d_workspace_bytes(C.byref(desc(L, row))))
    assert full >= 0
    if row.ws:
        return full
    out = (C.c_int64 * 24)()
    with call_env(row, RH_WGRAD2D_X6=0):
        L.check(L.lib.rh_conv2d_instance_info(C.byref(desc(L, row)), 2, 0, int(row.off == 0), 1, full, out), "instance_info")
    return int(out[12] + out[13])


def instance_info(L, row, **more):
    """The 24 numbers of rh_conv2d_instance_info for the call of ``row`` (under the row's switches, plus ``more``)."""
    out = (C.c_int64 * 24)()
    nbytes = workspace_bytes(L, row)
    with call_env(row, **more):
        L.check(L.lib.rh_conv2d_instance_info(C.byref(desc(L, row)), row.which, int(row.armed), int(row.off == 0), 1, nbytes, out),
                "instance_info")
    return tuple(out)


def kernel_of(info):
    return KERNELS[info[0]] if 0 <= info[0] < len(KERNELS) else None


def key_of(info, which):
    k = kernel_of(info)
    if k == "x6":
        return (k, which) + tuple(info[1:4])
    if k in ("dma", "igemm"):
        return (k, which) + tuple(info[1:5])
    if k == "smallm":
        return (k,) + tuple(info[1:4])
    if k in ("smallc", "wdma"):
        return (k, info[1])
    if k == "wx6":
        return (k, info[1], info[2])
    if k == "wgrad":
        return (k,) + tuple(info[1:5])
    return ("none",)


def fmt_key(key):
    if key[0] in ("x6", "dma", "igemm"):
        name = {"x6": "conv2d_x6_kernel", "dma": "conv2d_dma_kernel", "igemm": "conv2d_igemm_kernel"}[key[0]]
        return f"{name}<{', '.join(map(str, key[2:]))}> {'data gradient' if key[1] else 'forward'}"
    name = {"smallm": "conv2d_smallm_kernel", "smallc": "conv2d_smallc_fwd_kernel", "wx6": "wgrad2d_x6_kernel", "wdma": "wgrad2d_dma_kernel",
            "wgrad": "wgrad2d_kernel", "none": "nothing"}[key[0]]
    return f"{name}<{', '.join(map(str, key[1:]))}>"


def plan(info, which):
    """The plan part of the diagnostic by name."""
    if which < 2:
        n = "TR TQ nb PH PW ck phases gx gy gz lds tiles_r tiles_q family no_dma"
    else:
        n = "TR TQ Z chunks_per_z groups nc_max lds ws_used bias_ws total PH PW _ family short"
    return dict(zip(n.split(), info[5:]))


def phases(geo):
    """Per output phase of the data gradient (build_plan2, restated): the number of taps."""
    B, Ci, Co, H, W, k, s, dil, pad = geo
    out = []
    for ah in range(s[0]):
        for aw in range(s[1]):
            nh = sum(1 for th in range(k[0]) if (ah + pad[0] - th * dil[0]) % s[0] == 0)
            nw = sum(1 for tw in range(k[1]) if (aw + pad[1] - tw * dil[1]) % s[1] == 0)
            out.append(nh * nw)
    return out


def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def edges(row, info):
    """Names of the edges of the staging / tile addressing this call sits on, from the diagnostic's numbers and the geometry."""
    B, Ci, Co, H, W, k, s, dil, pad = row.geo
    ho, wo = out_hw(row.geo)
    kind, pl = kernel_of(info), plan(info, row.which)
    e = set()
    e.add("four paddings" if pad[0] and pad[1] else ("no padding" if not (pad[0] or pad[1]) else "padding in one dimension"))
    if dil[0] > 1 or dil[1] > 1:
        e.add("dilation in " + ("both" if dil[0] > 1 and dil[1] > 1 else ("H" if dil[0] > 1 else "W")))
    if s[0] > 1 or s[1] > 1:
        e.add("stride in " + ("both" if s[0] > 1 and s[1] > 1 else ("H" if s[0] > 1 else "W")))
    if k == (1, 1):
        e.add("1x1 kernel")
    if k[0] % 2 == 0 or k[1] % 2 == 0:
        e.add("even kernel")
    if W == 1 and wo == 1:
        e.add("W = 1")
    if row.which < 2:
        C_, M = (Ci, Co) if row.which == 0 else (Co, Ci)
        rows, qcols = (ho, wo) if row.which == 0 else (-(-H // s[0]), -(-W // s[1]))
        if rows % pl["TR"]:
            e.add("partial last row tile")
        if qcols % pl["TQ"]:
            e.add("partial last column tile")
        if pl["nb"] > 1 and B % pl["nb"]:
            e.add("nb > 1, B % nb != 0")
        if kind in ("x6", "dma", "igemm"):
            bm = 32 * info[1] * (info[3] if kind != "x6" else 1)
            if M % bm:
                e.add("M % row tile != 0")
            if M == 1:
                e.add("M = 1 in a 32-row tile")
            if kind == "x6":
                e.add("one 16-channel chunk" if C_ == 16 else "several 16-channel chunks")
                if row.which == 0:
                    e.add("epilogue: " + ("bias + LeakyReLU" if row.bias and row.act else ("bias" if row.bias else ("LeakyReLU" if row.act else "plain"))))
            else:
                if C_ % pl["ck"]:
                    e.add("C % ck != 0")
                if kind == "igemm":
                    e.add("DMA declined: " + NO_DMA[pl["no_dma"]])
        else:
            e.add("activation: " + ("LeakyReLU" if row.act and row.which == 0 else "none"))
        if row.which == 1 and (s[0] > 1 or s[1] > 1):
            if 0 in phases(row.geo):
                e.add("phases without taps")
            if H % s[0] or W % s[1]:
                e.add("short last phase")
        if row.which == 1 and row.act:
            e.add("fused derivative")
    else:
        T = k[0] * k[1]
        e.add("Z > 1" if pl["Z"] > 1 else "Z == 1")
        if row.act:
            e.add("fused derivative")
        if kind == "wx6":
            e.add(f"TQ {pl['TQ']}")
            tq = pl["TQ"]
            tr = 128 // tq
            while tr > 1 and tr // 2 >= ho:
                tr >>= 1
            if pl["TR"] < tr:
                e.add("TR shrunk")
            if Ci in (2, 16, 32, 48):
                e.add(f"C {Ci}")
            if T in (27, 32):
                e.add(f"T {T}")
            if s[1] == 2:
                if any((tw * dil[1]) & 1 for tw in range(k[1])):
                    e.add("sw 2, odd tw*dw")
                if any(tw and not (tw * dil[1]) & 1 for tw in range(k[1])):
                    e.add("sw 2, even tw*dw")
            if pl["Z"] == pl["total"] and pl["Z"] < 256 // pl["groups"]:
                e.add("Z capped by the tile count")
            if ho % pl["TR"]:
                e.add("partial last row tile")
            if wo % pl["TQ"]:
                e.add("partial last column tile")
        else:
            if pl["total"] % pl["chunks_per_z"]:
                e.add("chunks_per_z does not divide the chunks")
            wk = max(2, min(_pow2ceil(wo), 64))
            nominal = min(max(256 // wk, 4), _pow2ceil(ho)) if kind == "wgrad" else max(128 // wk, 1)
            if pl["TR"] < nominal:
                e.add("rk shrunk")
            if ho % pl["TR"]:
                e.add("partial last row chunk")
            if wo % pl["TQ"]:
                e.add("partial last column chunk")
            if Co % (32 * info[1] * info[3]) if kind == "wgrad" else Co % 32:
                e.add("M % row tile != 0")
    return e


NO_DMA = ("", "fused derivative", "2 GB", "patch too large", "LDS", "grid", "switched off")     # conv2d_f32.hip: plan2_dma

GEOMETRY = ["partial last row tile", "partial last column tile", "nb > 1, B % nb != 0", "M % row tile != 0", "M = 1 in a 32-row tile",
            "four paddings", "no padding", "dilation in H", "dilation in W", "dilation in both", "stride in H", "stride in W", "stride in both",
            "W = 1", "1x1 kernel", "even kernel"]
DGRAD = ["phases without taps", "short last phase"]
SMALL = ["partial last row tile", "partial last column tile", "four paddings", "no padding", "dilation in W", "W = 1", "1x1 kernel",
         "even kernel", "activation: LeakyReLU", "activation: none"]
WGRAD_F0 = ["Z > 1", "Z == 1", "chunks_per_z does not divide the chunks", "rk shrunk", "partial last row chunk", "partial last column chunk",
            "four paddings", "no padding", "dilation in H", "dilation in W", "dilation in both", "stride in H", "stride in W", "stride in both",
            "M % row tile != 0", "W = 1", "1x1 kernel", "even kernel"]
REQUIRED = {
    "x6": GEOMETRY + DGRAD + ["one 16-channel chunk", "several 16-channel chunks", "epilogue: bias + LeakyReLU", "epilogue: bias",
                              "epilogue: LeakyReLU", "epilogue: plain"],
    "dma": GEOMETRY + DGRAD + ["C % ck != 0"],
    "igemm": GEOMETRY + DGRAD + ["C % ck != 0", "fused derivative", "DMA declined: fused derivative", "DMA declined: patch too large",
                                 "DMA declined: LDS"],
    "smallm": SMALL,
    "smallc": SMALL,
    "wx6": ["TQ 8", "TQ 16", "TQ 32", "TR shrunk", "C 2", "C 16", "C 32", "C 48", "T 27", "T 32", "sw 2, odd tw*dw", "sw 2, even tw*dw", "Z > 1",
            "Z == 1", "Z capped by the tile count", "partial last row tile", "partial last column tile", "four paddings", "no padding",
            "dilation in H", "dilation in W", "dilation in both", "stride in H", "stride in W", "stride in both", "even kernel", "1x1 kernel"],
    "wdma": WGRAD_F0,
    "wgrad": WGRAD_F0 + ["fused derivative"],
}
# (kind, edge) pairs of REQUIRED that do not exist, with the reason read from the planner
_KH39 = "rh_conv2d_small{m,c_fwd}_eligible take kh = 3 or 9 only"
NOT_APPLICABLE = {
    ("smallm", "1x1 kernel"): _KH39,
    ("smallc", "1x1 kernel"): _KH39,
}


def seed(name):
    """Python's hash() is salted per process: a plain checksum of the row's name."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def make_name(which, geo, act, bias, off, env, armed, ws):
    B, Ci, Co, H, W, k, s, dil, pad = geo
    sw = " ".join(f"{n[len('RH_'):]}={v}" for n, v in env)
    return (f"{('fwd', 'dgrad', 'wgrad')[which]} {Ci}->{Co} k{k[0]}x{k[1]}{f' s{s[0]}x{s[1]}' if s != (1, 1) else ''}"
            f"{f' d{dil[0]}x{dil[1]}' if dil != (1, 1) else ''} B{B} {H}x{W} p{pad[0]},{pad[1]}{f' [{act}]' if act else ''}{' +b' if bias else ''}"
            f"{f' off{off}' if off else ''}{f' {sw}' if sw else ''}{'' if armed else ' unarmed'}{'' if ws else ' ws withheld'}")


# (which, geo, act, bias, off, env, armed, ws, key): printed by tests/conv2d_matrix_search.py
_X6, _SMALLM, _CX6, _WX6 = PER_CALL
_TABLE = [
    (0, (5, 32, 2, 5, 1, (3, 2), (2, 2), (2, 1), (3, 1)), '', False, 4, (), False, True, ('dma', 0, 1, 2, 1, 4)),
    (0, (1, 1, 40, 5, 1, (1, 1), (2, 2), (4, 4), (0, 0)), 'L', False, 0, (), True, True, ('dma', 0, 2, 1, 1, 4)),
    (0, (1, 3, 70, 1, 3, (1, 1), (2, 2), (2, 1), (0, 0)), '', True, 4, ((_WX6, 0),), True, True, ('dma', 0, 2, 2, 2, 2)),
    (0, (1, 1, 96, 7, 6, (1, 1), (4, 2), (1, 4), (0, 0)), '', False, 0, ((_WX6, 0),), True, True, ('dma', 0, 3, 1, 1, 4)),
    (1, (1, 1, 3, 11, 8, (1, 1), (1, 3), (2, 2), (0, 0)), '', False, 0, (), True, True, ('dma', 1, 1, 2, 1, 4)),
    (1, (1, 48, 32, 7, 6, (3, 2), (4, 1), (1, 2), (1, 1)), '', False, 0, (), False, True, ('dma', 1, 2, 1, 1, 4)),
    (1, (1, 70, 2, 1, 5, (1, 1), (4, 2), (1, 1), (0, 0)), '', False, 0, ((_SMALLM, 0),), True, True, ('dma', 1, 2, 2, 2, 2)),
    (1, (1, 96, 1, 5, 1, (3, 1), (2, 2), (1, 2), (1, 0)), '', False, 4, ((_CX6, 0),), True, True, ('dma', 1, 3, 1, 1, 4)),
    (0, (2, 24, 8, 1, 1, (1, 1), (1, 2), (1, 4), (0, 0)), 'L', True, 0, (), True, True, ('igemm', 0, 1, 2, 1, 4)),
    (0, (1, 3, 40, 16, 20, (9, 3), (4, 2), (4, 4), (17, 5)), '', False, 0, ((_WX6, 0),), True, True, ('igemm', 0, 2, 1, 1, 4)),
    (0, (1, 2, 100, 1, 1, (1, 1), (3, 2), (2, 1), (0, 0)), '', False, 0, (), True, True, ('igemm', 0, 2, 2, 2, 2)),
    (0, (2, 8, 96, 1, 1, (1, 1), (1, 3), (2, 1), (0, 0)), 'L', False, 4, ((_CX6, 0),), True, True, ('igemm', 0, 3, 1, 1, 4)),
    (1, (3, 1, 3, 16, 3, (2, 2), (3, 1), (2, 2), (2, 2)), 'L', False, 4, (), True, True, ('igemm', 1, 1, 2, 1, 4)),
    (1, (1, 48, 2, 11, 1, (5, 1), (2, 2), (2, 1), (4, 0)), 'L', False, 0, (), True, True, ('igemm', 1, 2, 1, 1, 4)),
    (1, (3, 70, 1, 5, 1, (1, 1), (3, 1), (2, 1), (0, 0)), 'L', False, 0, ((_WX6, 0),), True, True, ('igemm', 1, 2, 2, 2, 2)),
    (1, (1, 96, 1, 1, 3, (1, 1), (4, 2), (1, 2), (0, 0)), 'L', False, 4, ((_X6, 0), (_SMALLM, 0)), True, True, ('igemm', 1, 3, 1, 1, 4)),
    (0, (1, 2, 24, 16, 1, (3, 1), (1, 1), (1, 4), (0, 0)), 'L', True, 4, (), True, True, ('smallc', 3)),
    (0, (2, 1, 5, 5, 16, (9, 2), (1, 1), (1, 2), (4, 1)), '', False, 4, (), True, True, ('smallc', 9)),
    (0, (1, 1, 1, 9, 5, (3, 4), (1, 1), (1, 1), (1, 1)), 'L', True, 0, (), True, True, ('smallm', 3, 1, 0)),
    (1, (1, 1, 3, 7, 3, (3, 2), (1, 1), (1, 2), (0, 0)), '', False, 4, ((_X6, 0),), True, True, ('smallm', 3, 1, 1)),
    (0, (1, 2, 2, 7, 5, (3, 2), (1, 1), (1, 1), (1, 0)), 'L', True, 4, (), True, True, ('smallm', 3, 2, 0)),
    (1, (1, 2, 2, 5, 8, (3, 2), (1, 1), (1, 1), (0, 0)), '', False, 0, (), True, True, ('smallm', 3, 2, 1)),
    (0, (1, 1, 4, 7, 6, (3, 1), (1, 1), (1, 4), (0, 0)), 'L', True, 0, ((_WX6, 0),), True, True, ('smallm', 3, 4, 0)),
    (1, (2, 4, 1, 16, 1, (3, 1), (1, 1), (1, 1), (1, 0)), '', False, 4, (), True, True, ('smallm', 3, 4, 1)),
    (0, (1, 2, 1, 11, 3, (9, 2), (1, 1), (1, 1), (0, 0)), 'L', False, 0, ((_X6, 0),), True, True, ('smallm', 9, 1, 0)),
    (1, (3, 1, 1, 7, 6, (9, 2), (1, 1), (1, 1), (4, 0)), '', False, 4, ((_X6, 0),), True, True, ('smallm', 9, 1, 1)),
    (0, (3, 1, 2, 5, 1, (9, 2), (1, 1), (1, 1), (5, 1)), '', False, 0, ((_CX6, 0),), True, True, ('smallm', 9, 2, 0)),
    (1, (5, 2, 4, 5, 3, (9, 3), (1, 1), (1, 1), (4, 0)), '', False, 0, (), True, True, ('smallm', 9, 2, 1)),
    (0, (1, 2, 3, 40, 3, (9, 2), (1, 1), (1, 1), (0, 0)), '', True, 0, (), True, True, ('smallm', 9, 4, 0)),
    (1, (1, 4, 2, 7, 6, (9, 2), (1, 1), (1, 1), (5, 1)), '', False, 0, (), True, True, ('smallm', 9, 4, 1)),
    (2, (3, 24, 16, 5, 1, (1, 1), (3, 1), (2, 1), (0, 0)), '', False, 0, (), True, False, ('wdma', 1)),
    (2, (3, 32, 32, 16, 100, (3, 2), (2, 2), (3, 2), (4, 2)), '', False, 0, (), False, True, ('wdma', 2)),
    (2, (2, 64, 4, 11, 1, (5, 1), (1, 3), (1, 2), (3, 1)), '', False, 0, ((_X6, 0),), True, True, ('wdma', 4)),
    (2, (3, 100, 8, 65, 1, (1, 1), (2, 1), (2, 1), (0, 0)), 'L', True, 0, ((_SMALLM, 0),), True, True, ('wgrad', 1, 2, 1, 4)),
    (2, (2, 2, 64, 1, 3, (1, 1), (3, 1), (1, 4), (0, 0)), 'L', True, 0, ((_X6, 0), (_SMALLM, 0)), True, True, ('wgrad', 2, 1, 1, 4)),
    (2, (1, 2, 100, 7, 13, (2, 2), (4, 2), (2, 2), (1, 1)), 'L', True, 0, ((_SMALLM, 0),), True, True, ('wgrad', 2, 2, 2, 2)),
    (2, (1, 3, 96, 16, 5, (2, 2), (1, 3), (1, 4), (0, 0)), 'L', True, 4, (), False, True, ('wgrad', 3, 1, 1, 4)),
    (2, (1, 16, 4, 5, 8, (9, 3), (4, 1), (1, 2), (5, 3)), '', False, 4, (), True, True, ('wx6', 3, 1)),
    (2, (1, 2, 4, 11, 70, (1, 1), (1, 2), (3, 2), (0, 0)), '', True, 0, (), True, True, ('wx6', 3, 2)),
    (2, (3, 32, 4, 20, 13, (4, 8), (3, 2), (2, 1), (0, 0)), '', False, 4, (), True, True, ('wx6', 3, 2)),
    (2, (1, 48, 2, 5, 23, (3, 2), (1, 1), (3, 2), (4, 2)), '', True, 4, (), True, True, ('wx6', 6, 1)),
    (0, (1, 16, 24, 20, 16, (3, 2), (4, 1), (1, 2), (2, 2)), '', True, 0, (), True, True, ('x6', 0, 1, 1, 4)),
    (0, (2, 16, 1, 7, 1, (3, 1), (4, 2), (1, 1), (2, 1)), 'L', False, 0, (), True, True, ('x6', 0, 1, 1, 8)),
    (0, (5, 32, 5, 1, 1, (1, 1), (4, 1), (1, 2), (0, 0)), 'L', True, 0, ((_WX6, 0),), True, True, ('x6', 0, 1, 2, 4)),
    (0, (1, 16, 2, 129, 1, (2, 2), (1, 3), (2, 1), (2, 1)), '', False, 0, (), True, True, ('x6', 0, 1, 2, 8)),
    (0, (1, 16, 48, 33, 23, (3, 2), (4, 1), (1, 2), (0, 0)), '', False, 4, ((_WX6, 0),), True, True, ('x6', 0, 2, 1, 4)),
    (0, (1, 16, 40, 16, 5, (1, 1), (3, 2), (2, 1), (0, 0)), 'L', False, 0, (), True, True, ('x6', 0, 2, 1, 8)),
    (0, (1, 16, 48, 7, 1, (1, 1), (1, 1), (1, 1), (0, 0)), '', True, 4, ((_SMALLM, 0),), True, True, ('x6', 0, 2, 2, 4)),
    (0, (3, 16, 40, 9, 1, (1, 1), (4, 2), (2, 2), (0, 0)), 'L', True, 4, ((_WX6, 0),), True, True, ('x6', 0, 2, 2, 8)),
    (0, (1, 16, 70, 1, 5, (1, 1), (2, 2), (1, 1), (0, 0)), '', True, 0, (), True, True, ('x6', 0, 3, 1, 4)),
    (0, (1, 16, 70, 9, 6, (1, 1), (3, 2), (1, 1), (0, 0)), '', False, 0, ((_WX6, 0),), True, True, ('x6', 0, 3, 1, 8)),
    (1, (1, 2, 32, 5, 1, (4, 3), (1, 1), (1, 1), (2, 2)), '', False, 4, (), True, True, ('x6', 1, 1, 1, 8)),
    (1, (1, 1, 32, 9, 5, (1, 1), (3, 2), (4, 4), (0, 0)), '', False, 0, (), True, True, ('x6', 1, 1, 2, 4)),
    (1, (1, 1, 16, 5, 5, (2, 2), (2, 1), (4, 4), (0, 2)), '', False, 0, (), True, True, ('x6', 1, 1, 2, 8)),
    (1, (5, 128, 16, 1, 1, (3, 2), (2, 1), (1, 2), (2, 2)), '', False, 0, (), True, True, ('x6', 1, 2, 1, 8)),
    (1, (2, 64, 16, 1, 3, (1, 1), (4, 1), (1, 1), (0, 0)), '', False, 4, (), True, True, ('x6', 1, 2, 2, 4)),
    (1, (5, 40, 16, 1, 1, (3, 2), (1, 2), (1, 1), (2, 1)), '', False, 4, (), True, True, ('x6', 1, 2, 2, 8)),
    (1, (5, 96, 16, 1, 1, (1, 1), (1, 1), (1, 2), (0, 0)), '', False, 0, ((_WX6, 0),), True, True, ('x6', 1, 3, 1, 4)),
    (1, (1, 70, 32, 9, 100, (5, 1), (1, 3), (4, 4), (8, 0)), '', False, 4, ((_WX6, 0),), True, True, ('x6', 1, 3, 1, 8)),
]
ROWS = [Row(make_name(*t[:8]), *t) for t in _TABLE]
assert len({r.name for r in ROWS}) == len(ROWS)

# instances no call can select through the C ABI under the default planner, with the reason: (key, reason)
_DGRAD_TN1 = ("a data gradient gathers at stride 1, so the 256-column tile's patch is at most twice the 128-column one's: with P <= 512 "
              "(NQ = 4) it passes both the 2 P <= 2048 rule and the 80 KB rule of plan_c2x, which then prefers TN = 2")
UNREACHABLE = [(("x6", 1, 1, 1, 4), _DGRAD_TN1), (("x6", 1, 2, 1, 4), _DGRAD_TN1)]
