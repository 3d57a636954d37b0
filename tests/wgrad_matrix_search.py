"""Finds the rows of tests/wgrad_matrix.py (a command-line helper, not a test; no GPU: it only asks
rh_conv1d_bwd_weight_instance_info).

    python tests/wgrad_matrix_search.py [samples]

draws small random calls (fixed seed), asks the diagnostic which instance each launches and which edges it sits on, and covers
every instance of wgrad_matrix.x6_instances() / f0_instances() and every (kind, edge) pair of wgrad_matrix.REQUIRED greedily: the
call that adds the most new conditions, cheapest first among equals.  Prints literal lines of ``_TABLE`` and what stayed uncovered
(candidates for wgrad_matrix.UNREACHABLE / NOT_APPLICABLE).  After a planner change that re-routes rows, run it again.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the package, from the repository tree
import wgrad_matrix as W  # noqa: E402

M_ROWS = (32, 40, 64, 70, 80, 96, 100, 128, 144, 160, 192, 200, 256)
CHANNELS = (8, 10, 16, 22, 24, 32, 43, 48, 54, 64, 80, 86, 96)
LENGTHS = (20, 28, 31, 32, 60, 64, 70, 96, 100, 127, 128, 150, 224, 257, 300)
ENVS = ((), (("RH_WGRAD_X6_PLANES", 1),), (("RH_WGRAD_X6_PLANES", 0),), (("RH_WGRAD_X6_WIDE", 0),), (("RH_WGRAD_X6_BLOCKS", 1),),
        (("RH_WGRAD_X6_BLOCKS", 2),), (("RH_WGRAD_X6_PLANES", 1), ("RH_WGRAD_X6_BLOCKS", 1)), (("RH_WGRAD_X6", 0),), (("RH_WGRAD_X6", 0),))


def draw(rng):
    tr = rng.random() < 0.2
    s = rng.choice((2, 4)) if tr or rng.random() < 0.2 else 1
    if s > 1:
        k, dil = rng.choice((s, 2 * s)), 1
    else:
        k, dil = rng.choice(((1, 1), (3, 1), (3, 1), (3, 9), (3, 9), (3, 13), (7, 1)))
    span = (k - 1) * dil
    if tr:
        p = rng.choice((0, (k - s) // 2))
        pad = (p, p)
    else:
        pad = rng.choice(((0, 0), (span, 0), (0, span), (span // 2, span - span // 2)))
    m, c = rng.choice(M_ROWS), rng.choice(CHANNELS)
    geo = (rng.choice((1, 2, 3, 5)), m if tr else c, c if tr else m, rng.choice(LENGTHS), k, s, dil, pad, tr)
    act = rng.choice(("", "L", "L", "S") if rng.random() < 0.15 else ("", "L"))
    return geo, act, rng.random() < 0.5, rng.choice((0, 0, 4)), rng.choice(ENVS), True


def features(L, cand):
    geo, act, bias, off, env, armed = cand
    if geo[3] <= (geo[4] - 1) * geo[6] or W.out_len(geo) < 1:        # every tap reads data somewhere
        return None
    row = W.Row("", geo, act, bias, off, env, armed, None)
    info = W.instance_info(L, row)
    if info[0] not in (0, 1):
        return None
    key, kind = W.key_of(info), W.kind_of(info)
    f = {("inst", key)}
    if kind is not None:
        f |= {(kind, e) for e in W.edges(row, info) if e in W.REQUIRED[kind]}
    return key, frozenset(f)


def main(argv):
    from rave_amd import _lib as L
    W.assert_default_planner_env()
    rng = random.Random(20)
    best = {}                                   # feature set -> cheapest candidate
    for _ in range(int(argv[0]) if argv else 400000):
        cand = draw(rng)
        got = features(L, cand)
        if got is None:
            continue
        B, Ci, Co, Lx, k = cand[0][:5]
        cost = B * Ci * Co * Lx * k
        if got[1] not in best or cost < best[got[1]][0]:
            best[got[1]] = (cost, cand, got[0])
    want = {("inst", i) for i in W.x6_instances() + W.f0_instances()}
    want |= {(kind, e) for kind, es in W.REQUIRED.items() for e in es if (kind, e) not in W.NOT_APPLICABLE}
    chosen = []
    while want:
        gain, cost, f = max(((len(f & want), -c[0], f) for f, c in best.items()), key=lambda t: t[:2])
        if gain == 0:
            break
        want -= f
        chosen.append(best[f])
    for cost, (geo, act, bias, off, env, armed), key in sorted(chosen, key=lambda t: (t[2], t[0])):
        print(f"    ({geo}, {act!r}, {bias}, {off}, {env}, {armed}, {key}),")
    print(f"# {len(chosen)} rows; uncovered:", file=sys.stderr)
    for w in sorted(want, key=str):
        print(f"#   {w}", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
