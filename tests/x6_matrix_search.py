"""Finds rows for the table of tests/x6_matrix.py (a command-line helper, not a test; no GPU: it only asks rh_conv1d_plan_info).

    python tests/x6_matrix_search.py IS=2 which=0 kmode=combine "edge=B % nb != 0" [n=5]

enumerates small geometries (and the few long ones the 64-column wave tile needs), derives the instance key and the edges of
each with the helpers of x6_matrix, keeps those whose key fields equal every FIELD=VALUE given (fields of x6_matrix.Key; ``edge=``
may be repeated) and prints the ``n`` cheapest (by multiply-adds) as literal lines of ``_TABLE``.  The table was made by calling
this for every condition tests/test_x6_matrix_host.py asserts, cheapest row first, and -- for each of the 30 tile shapes -- for
the plain modes 0 and 5 (forward) and the derivative mode 2 (data gradient); after a planner change that re-routes a row, ask
again for the key the row used to have.
"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the package, from the repository tree
import x6_matrix as X  # noqa: E402

CHANNELS = (4, 8, 16, 20, 24, 32, 48, 64, 80, 96, 128, 144, 160, 176, 192)
BATCHES = (1, 2, 3, 5, 9)
LENGTHS = (1, 2, 3, 4, 31, 33, 63, 65, 124, 129, 257, 8325, 24600, 49157, 98309, 196615, 393231)
OPS = {0: ("", "b", "a", "ba", "bo", "bao", "L", "Lb", "La", "Lba"), 1: ("", "L", "a", "La")}


def geometries(which, stride, long, dilated):
    """``long``: with the lengths only the 64-column wave tile needs; ``dilated``: with the dilations around the LDS bound."""
    for tr in ((False,) if stride == 1 else (False, True)):
        ks = (1, 2, 3, 5, 7, 17) if stride == 1 else (stride, 2 * stride, 2 * stride + 1, 34)
        dils = (1, 2, 9, 64, 65, 128, 129) if dilated else (1,)
        for B, Ci, Co, Lx, k, dil in itertools.product(BATCHES, CHANNELS, CHANNELS, [n for n in LENGTHS if long or n <= 257], ks, dils):
            span = (k - 1) * dil
            for pad in {(0, 0), (span, 0), (span // 2, span - span // 2), (span + 2, 0)}:
                geo = (B, Ci, Co, Lx, k, stride, dil, pad, tr)
                if (not tr or pad[0] < k) and X.out_len(geo) >= 1:
                    yield geo


def main(argv):
    from rave_amd import _lib as L
    want = [a.split("=", 1) for a in argv]
    n = int(dict(want).get("n", 5))
    edges = [v for f, v in want if f == "edge"]
    fields = {f: v for f, v in want if f not in ("edge", "n")}
    assert set(fields) <= set(X.Key._fields), fields
    found = []
    for which in (0, 1):
        if fields.get("which", str(which)) != str(which):
            continue
        # the operands follow from the mode asked for; none asked for = the plain call
        modes = [o for o in OPS[which] if all(fields.get(f, str(v)) == str(v) for f, v in
                 (("leaky", which == 0 and "L" in o), ("epi", X.operand_mode(X.Row("", which, None, o, True, None, None)))))]
        for stride, ops in itertools.product((1, 2, 4), modes if {"leaky", "epi"} & set(fields) else modes[:1]):
            for geo in geometries(which, stride, long="tn" not in fields or fields["tn"] == "2", dilated=stride == 1 and bool(edges)):
                B, Ci, Co, Lx, k = geo[:5]
                if B * Ci * Co * Lx * k > 4e9:
                    continue
                probe = X.Row("", which, geo, ops, True, None, None)
                info = X.plan_info(L, probe)
                if info[0] != 1 or any(f in fields and fields[f] != str(v) for f, v in zip(("tm", "tn", "wm", "", "IS", "vs"), info[1:7])):
                    continue
                if not set(edges) <= X.edges(probe, info):
                    continue
                for ws, combine in itertools.product((True, False), (None, 1)):
                    row = probe._replace(ws=ws, combine=combine)
                    key = X.derive_key(L, row)
                    if key is not None and all(str(getattr(key, f)) == v for f, v in fields.items()):
                        found.append((B * Ci * Co * Lx * k, row, key))
                        break
    for _, row, key in sorted(found, key=lambda t: t[0])[:n]:
        print(f"    ({row.which}, {row.geo}, {row.ops!r}, {row.ws}, {row.combine}, {tuple(key)}),")


if __name__ == "__main__":
    main(sys.argv[1:])
