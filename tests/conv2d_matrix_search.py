"""Finds the rows of tests/conv2d_matrix.py (a command-line helper, not a test; no GPU: it only asks rh_conv2d_instance_info).

    python tests/conv2d_matrix_search.py [samples]

draws small random calls (fixed seed), asks the diagnostic which instance each launches and which edges it sits on, and covers every
instance of conv2d_matrix.instances() and every (kernel, edge) pair of conv2d_matrix.REQUIRED greedily: the call that adds the most new
conditions, cheapest first among equals.  Prints literal lines of ``_TABLE`` and what stayed uncovered (candidates for
conv2d_matrix.UNREACHABLE / NOT_APPLICABLE).  After a planner change that re-routes rows, run it again.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the package, from the repository tree
import conv2d_matrix as M  # noqa: E402

CHANNELS = (1, 2, 3, 4, 5, 8, 16, 16, 24, 32, 32, 40, 48, 64, 70, 96, 100, 128, 160)
HEIGHTS = (1, 5, 7, 9, 11, 16, 19, 20, 33, 40, 65, 70, 129)
WIDTHS = (1, 3, 5, 6, 8, 13, 16, 20, 23, 26, 29, 33, 40, 61, 70, 100, 130)
KERNELS = ((1, 1), (3, 3), (3, 3), (9, 3), (9, 3), (3, 9), (3, 9), (5, 1), (2, 2), (4, 3), (3, 2), (3, 1), (4, 8), (9, 7), (3, 4), (9, 2))
STRIDES = ((1, 1), (1, 1), (1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (3, 2), (4, 1), (1, 3), (4, 2))
DILS = ((1, 1), (1, 1), (1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (4, 4), (3, 2))
ENVS = ((), (), (), (("RH_CONV2D_X6", 0),), (("RH_CONV2D_SMALLM", 0),), (("RH_CONV_X6", 0),), (("RH_WGRAD2D_X6", 0),),
        (("RH_CONV2D_X6", 0), ("RH_CONV2D_SMALLM", 0)))


def draw(rng):
    k, s, dil = rng.choice(KERNELS), rng.choice(STRIDES), rng.choice(DILS)
    span = ((k[0] - 1) * dil[0], (k[1] - 1) * dil[1])
    pad = rng.choice(((0, 0), (span[0] // 2, span[1] // 2), (span[0] // 2, 0), (0, span[1] // 2), (span[0] // 2 + 1, span[1] // 2 + 1)))
    geo = (rng.choice((1, 2, 3, 5)), rng.choice(CHANNELS), rng.choice(CHANNELS), rng.choice(HEIGHTS), rng.choice(WIDTHS), k, s, dil, pad)
    which = rng.choice((0, 1, 2))
    act = "L" if rng.random() < (0.5 if which == 0 else 0.15) else ""
    return (which, geo, act, which != 1 and rng.random() < 0.5, rng.choice((0, 0, 4)), rng.choice(ENVS), rng.random() < 0.9,
            which != 2 or rng.random() < 0.85)


def features(L, cand):
    which, geo, act, bias, off, env, armed, ws = cand
    if not M.valid(geo) or max(M.numels(geo)) > M.MAX_NUMEL:
        return None
    # every tap reads data somewhere, so that no slice of a weight gradient is identically zero
    if (geo[5][0] - 1) * geo[7][0] >= geo[3] + geo[8][0] or (geo[5][1] - 1) * geo[7][1] >= geo[4] + geo[8][1]:
        return None
    row = M.Row("", which, geo, act, bias, off, env, armed, ws, None)
    try:
        info = M.instance_info(L, row)
    except RuntimeError:                         # (no kernel takes this geometry: the call returns RH_ERR_UNSUPPORTED)
        return None
    kind = M.kernel_of(info)
    if kind is None or (which == 2 and M.plan(info, 2)["short"]):
        return None
    key = M.key_of(info, which)
    f = {("inst", key)} | {(kind, e) for e in M.edges(row, info) if e in M.REQUIRED[kind]}
    # the silent fallbacks, each by the kernel that then runs
    if kind in ("dma", "igemm", "wdma", "wgrad") and not env:
        twin = M.kernel_of(M.instance_info(L, row._replace(armed=True, ws=True)))
        if not armed and twin in ("x6", "wx6"):
            f.add(("fallback", "unarmed", which))
        if which == 2 and armed and not ws and twin == "wx6":
            f.add(("fallback", "ws withheld"))
        if (geo[2] if which == 1 else geo[1]) % 16 and which < 2:
            f.add(("fallback", "C % 16", kind))
    if act and (which == 1 or (which == 2 and bias)):
        f.add(("fused", which, key))
    if kind == "wx6" and M.numels(geo)[2] >= 4096:          # large enough for the GPU test to demand other bits than family 0
        f.add(("wx6", "4096 weights"))
    return key, frozenset(f)


def wanted():
    want = {("inst", i) for i in M.instances()}
    want |= {(kind, e) for kind, es in M.REQUIRED.items() for e in es if (kind, e) not in M.NOT_APPLICABLE}
    return want


def main(argv):
    from rave_amd import _lib as L
    M.assert_default_planner_env()
    rng = random.Random(20)
    best = {}                                   # feature set -> cheapest candidate
    for _ in range(int(argv[0]) if argv else 300000):
        cand = draw(rng)
        got = features(L, cand)
        if got is None:
            continue
        cost = sum(M.numels(cand[1])) * (1 + cand[1][5][0] * cand[1][5][1] // 8)
        if got[1] not in best or cost < best[got[1]][0]:
            best[got[1]] = (cost, cand, got[0])
    want = wanted()
    want |= {f for fs in best for f in fs if f[0] in ("fallback", "fused") or f == ("wx6", "4096 weights")}
    chosen = []
    while want:
        gain, cost, f = max(((len(f & want), -c[0], f) for f, c in best.items()), key=lambda t: t[:2])
        if gain == 0:
            break
        want -= f
        chosen.append(best[f])
    for cost, cand, key in sorted(chosen, key=lambda t: (str(t[2]), t[0])):
        print(f"    {cand + (key,)},")
    print(f"# {len(chosen)} rows; uncovered:", file=sys.stderr)
    for w in sorted(want, key=str):
        print(f"#   {w}", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
