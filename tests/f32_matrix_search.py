"""Finds the rows of tests/f32_matrix.py (a command-line helper, not a test; no GPU: it only asks rh_conv1d_f32_instance_info).

    python tests/f32_matrix_search.py cover [draws=300000] [seed=1]
    python tests/f32_matrix_search.py TM=3 kmode=finalize4 "edge=C odd" [n=5]

``cover`` draws small random calls (sequences up to a few hundred positions, batch <= 5, channels <= 200), adds the sweeps over one long
staged row (B = 1, 2 - 4 channels, k = 2, growing dilation) that cross the DMA-slot, 20-bit-reciprocal and LDS bounds of plan_dma for
each tile shape, collects the coverage conditions each call meets (f32_matrix.tags_of) and prints a greedy cover of
f32_matrix.required() as literal lines of ``_TABLE``: for each condition still open the cheapest call (by multiply-adds) that meets
it.  Conditions no call met are printed behind the table.  The second form lists the ``n`` cheapest drawn calls whose key fields equal
every FIELD=VALUE given (fields of f32_matrix.Key; ``edge=`` may be repeated); after a planner change that re-routes a row, ask
again for the key the row used to have.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the package, from the repository tree
import f32_matrix as X  # noqa: E402

CHANNELS = (3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 48, 64, 80, 96, 100, 130, 160, 200)
LENGTHS = (1, 2, 3, 5, 8, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 257)
OPS = {0: ("", "b", "a", "ba", "bo", "bao", "L", "Lb", "Lba", "Lbo", "S", "Sb", "Sba"), 1: ("", "L", "S", "a", "La", "Sa")}


def cost(geo):
    B, Ci, Co, Lx, k, s, dil, pad, tr, inner, in_valid = geo
    return B * Ci * Co * max(Lx, X.out_len(geo)) * k * inner


def draw(rng):
    which = rng.randrange(2)
    tr = rng.random() < 0.25
    s = rng.choice((1, 1, 1, 2, 3, 4))
    k = rng.choice((1, 2, 3, 5, 7) if s == 1 else (s, s + 1, 2 * s, 2 * s + 1))
    dil = 1 if (tr or (s > 1 and which == 1)) else rng.choice((1, 1, 2, 9))
    inner = 1 if tr else rng.choice((1, 1, 1, 2, 3, 5))
    Lx = rng.choice(LENGTHS)
    span = (k - 1) * dil
    pad = rng.choice(((0, 0), (span, 0), (span // 2, span - span // 2), (span + 2, 0)))
    if tr and pad[0] >= k:
        pad = (0, 0)
    in_valid = 0
    if inner > 1 and Lx > 1 and rng.random() < 0.7:
        in_valid = Lx * inner - rng.randrange(1, inner)
    geo = (rng.choice((1, 1, 2, 3, 5)), rng.choice(CHANNELS), rng.choice(CHANNELS), Lx, k, s, dil, pad, tr, inner, in_valid)
    return X.Row("", which, geo, rng.choice(OPS[which]), rng.choice((16, 16, 4)), rng.random() < 0.8, None)


def sweeps():
    """One long staged row per tile shape: k = 2 taps a dilation apart, just enough positions for a full column tile."""
    for which, (Ci, Co) in ((0, (2, 24)), (0, (2, 40)), (0, (2, 80)), (0, (2, 100)), (0, (4, 24)), (0, (4, 40)), (0, (4, 80)), (0, (4, 100))):
        for ncols in (128, 256):
            for dil in list(range(1400, 4200)) + list(range(9000, 10400)):
                geo = (1, Ci, Co, ncols + dil, 2, 1, dil, (0, 0), False, 1, 0)
                yield X.Row("", which, geo, "b", 16, True, None)
                if Ci == 2 and 2700 <= dil < 3000:      # one padded position: the tile origin moves down 4, the row's last float4 is read
                    yield X.Row("", which, (1, Ci, Co, ncols - 1 + dil, 2, 1, dil, (1, 0), False, 1, 0), "b", 16, True, None)


def live(row):
    """At least half of the output columns read an input position that exists: the GPU test wants no output near zero in norm."""
    g = X.gemm(row)
    npos = -(-g["in_row"] // g["inner"])
    ok = sum(any(0 <= n * g["istr"] + o < npos for o in ph) for ph in g["offs"] for n in range(min(g["rows"], 512)))
    return 2 * ok >= len(g["offs"]) * min(g["rows"], 512)


def candidates(L, draws, seed_):
    rng = random.Random(seed_)
    seen = set()
    for row in [draw(rng) for _ in range(draws)] + list(sweeps()):
        sig = (row.which, row.geo, row.ops, row.align, row.ws)
        if sig in seen or X.out_len(row.geo) < 1 or cost(row.geo) > 3e8 or not live(row):
            continue
        seen.add(sig)
        try:
            tags = X.tags_of(L, row)
        except RuntimeError:                # a descriptor the library refuses
            continue
        if tags:
            yield row, tags


def main(argv):
    from rave_amd import _lib as L
    X.assert_default_planner_env()
    args = dict(a.split("=", 1) for a in argv if "=" in a and not a.startswith("edge="))
    pool = list(candidates(L, int(args.pop("draws", 300000)), int(args.pop("seed", 1))))
    if "cover" in argv:
        chosen, open_ = [], []
        have = set()
        # first the siblings of the sweeps: the last dilation on a bound and the next one, beyond it; and the smallest staged row
        # beyond the exact range of the slot reciprocal (two rows of 756 float4)
        sweep = {(r.geo[:3], r.geo[3] - r.geo[6], r.geo[6]): (r, t) for r, t in pool if r.geo[3] > 1000}
        for s in X.SHAPES:
            for a_edge, b_edge in (("last staged row that fits nx <= 8", "VEC refused for its DMA slots"),
                                   ("last geometry within 160 KiB of LDS", "DMA stages beyond 160 KiB of LDS: synchronous kernel")):
                # (a VEC row needs a memory row of a multiple of 4 elements: its next sibling is 4 positions on)
                step = 4 if a_edge.startswith("last staged") else 1
                fit = [(cost(r.geo), k) for k, (r, t) in sweep.items() if ("edge", s, a_edge) in t and
                       ("edge", s, b_edge) in sweep.get((k[0], k[1], k[2] + step), (None, ()))[1]]
                if not fit:
                    open_.append((s, a_edge, b_edge))
                    continue
                k = min(fit)[1]
                for row, tags in (sweep[k], sweep[(k[0], k[1], k[2] + step)]):
                    chosen.append(row)
                    have |= tags
            # (the widest of them: only the last float4 of the second row is lost, and only that row reads it)
            fit = [(r.geo[6], k) for k, (r, t) in sweep.items() if ("staged row beyond the exact range of the 20-bit reciprocal",) in t and
                   ("kmode", s, "unsplit") in t and X.vec_plan0(r, X.instance_info(L, r)) == (2, 756)]
            if fit:
                chosen.append(sweep[max(fit)[1]][0])
                have |= sweep[max(fit)[1]][1]
        for need in X.required():
            if need in have:
                continue
            fit = [(cost(r.geo), i) for i, (r, t) in enumerate(pool) if need in t]
            if not fit:
                open_.append(need)
                continue
            row, tags = pool[min(fit)[1]]
            chosen.append(row)
            have |= tags
        for row in chosen:
            print(f"    ({row.which}, {row.geo}, {row.ops!r}, {row.align}, {row.ws}, {tuple(X.derive_key(L, row))}),")
        for need in open_:
            print("# no call met:", need)
        return
    n = int(args.pop("n", 5))
    edges = [a.split("=", 1)[1] for a in argv if a.startswith("edge=")]
    assert set(args) <= set(X.Key._fields), args
    found = []
    for row, tags in pool:
        key = X.derive_key(L, row)
        if all(str(getattr(key, f)) == v for f, v in args.items()) and set(edges) <= {t[2] for t in tags if t[0] == "edge"}:
            found.append((cost(row.geo), row, key))
    for _, row, key in sorted(found, key=lambda t: t[0])[:n]:
        print(f"    ({row.which}, {row.geo}, {row.ops!r}, {row.align}, {row.ws}, {tuple(key)}),")


if __name__ == "__main__":
    main(sys.argv[1:])
