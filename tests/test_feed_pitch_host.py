"""Host side of the pitched data feed (rave_amd/data.py): the ratio list of RandomPitch (rave/transforms.py:56-89), the
polyphase tap table of scipy.signal.resample_poly, and the random draws.  No GPU: everything here is host logic."""
import bisect
import math

import numpy as np
import pytest
from scipy.signal import firwin

from rave_amd import data as D

RANGE = (0.7, 1.3)


def get_factors(factor_limit, pitch_range):
    """RandomPitch._get_factors (rave/transforms.py:63-75), restated."""
    factor_list, ratio_list = [], []
    for x in range(1, factor_limit):
        for y in range(1, factor_limit):
            if x == y:
                continue
            factor = x / y
            if factor <= pitch_range[1] and factor >= pitch_range[0]:
                i = bisect.bisect_left(factor_list, factor)
                factor_list.insert(i, factor)
                ratio_list.insert(i, (x, y))
    return factor_list, ratio_list


def reduced(ratio):
    g = math.gcd(*ratio)
    return ratio[0] // g, ratio[1] // g


def test_ratio_list_is_the_reference_one():
    factors, ratios = get_factors(20, RANGE)
    table = D.PitchTable(RANGE)
    assert table.factor_list == factors and table.ratio_list == ratios
    assert (2, 3) not in ratios and (3, 4) in ratios and (6, 8) in ratios          # unreduced duplicates are kept
    distinct = {reduced(r) for r in ratios}
    assert len(distinct) == 63 and max(max(r) for r in distinct) <= 19
    assert set(table.offset) == distinct
    # the pick of RandomPitch.__call__ (:81-87): bisect_left into the list with duplicates, clamped to the last entry
    for u in (0.0, 0.123, 0.5, 0.77, 0.999999, 1.0):
        for length, n in ((131072, 65536), (9001, 8000)):
            hi = min(RANGE[1], length / n)
            i = bisect.bisect_left(factors, u * (hi - RANGE[0]) + RANGE[0])
            assert table.pick(u, length, n) == ratios[min(i, len(ratios) - 1)]


def test_tap_table_is_the_filter_of_resample_poly():
    table = D.PitchTable(RANGE)
    end = 0
    for (up, down), off in sorted(table.offset.items(), key=lambda kv: kv[1]):
        m = max(up, down)
        h = up * firwin(2 * 10 * m + 1, 1 / m, window=("kaiser", 5.0))
        assert off == end                                                           # packed, no overlap
        got = table.taps[off:off + len(h)]
        assert got.dtype == np.float64 and np.abs(got - h).max() <= 1e-15, (up, down)
        end = off + len(h)
    assert end == len(table.taps)


def draw3(rng, n_items, length, batch, n_signal, sr, p_mangle):
    """The three draws of the unpitched feed, restated as they stand in GpuBatchFeed.draw before this feature."""
    items = rng.integers(0, n_items, batch)
    in_points = rng.integers(0, length - n_signal + 1, batch)
    angles = [D.random_angle(rng, 20, 2000, sr) if rng.random() < p_mangle else None for _ in range(batch)]
    return items, in_points, angles


@pytest.mark.parametrize("seed", [0, 7])
def test_unpitched_draws_consume_the_generator_as_before(seed):
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    for _ in range(3):                                                              # consecutive batches stay in step
        got = D.draw_batch(a, 11, 30000, 16, 8192, 44100, .8, None)
        ref = draw3(b, 11, 30000, 16, 8192, 44100, .8)
        assert len(got) == 3
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    # with pitch the first three draw in the same order: items and angles agree, in_points where the item is not pitched
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    items, in_points, angles, ratios = D.draw_batch(a, 11, 30000, 16, 8192, 44100, .8, D.PitchTable(RANGE))
    ref = draw3(b, 11, 30000, 16, 8192, 44100, .8)
    assert np.array_equal(items, ref[0]) and angles == ref[2]
    assert all(in_points[i] == ref[1][i] for i in range(16) if ratios[i] is None)


def test_pitched_draws_stay_inside_the_resampled_item():
    table = D.PitchTable(RANGE)
    rng = np.random.default_rng(3)
    length, n = 9001, 6000                                                          # 9001 * 0.7 = 6300.7: every ratio leaves room
    seen, at_edge = set(), 0
    for _ in range(40):
        items, in_points, angles, ratios = D.draw_batch(rng, 5, length, 32, n, 44100, .8, table)
        for p, r in zip(in_points, ratios):
            if r is None:
                assert 0 <= p <= length - n
                continue
            assert r in table.ratio_list
            up, down = reduced(r)
            n_out = -(-length * up // down)
            assert 0 <= p <= n_out - n, (p, r)
            seen.add(r)
            at_edge += p > length - n
    assert len(seen) > 30 and at_edge > 0          # about half the items pitched, over the list; crop points beyond L - n occur
    assert table.shortest(length) == math.ceil(length * 0.7)
