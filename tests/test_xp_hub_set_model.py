"""The numpy model behind tests/test_gpu_xp_hub_set.py (tests/xp_hub_set_model.py), on graphs small enough to work out by hand."""
import os
import sys

import numpy as np

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xp_hub_set_model as model  # noqa: E402

U64, I64 = np.uint64, np.int64


def graph(n, out):
    rows = np.concatenate([np.full(len(v), u, dtype=U64) for u, v in out.items()])
    cols = np.concatenate([np.asarray(v, dtype=U64) for v in out.values()])
    return oracle.build_csr(n, n, rows, cols)


def test_the_set_is_cut_at_the_quarter_rounded_up_and_ordered_by_degree_then_id():
    # degrees: 0 -> 9, 5 -> 3 (= ceil(9 / 4)), 3 -> 3, 7 -> 2, 2 -> 4
    a = graph(12, {0: range(1, 10), 5: [1, 2, 3], 3: [9, 10, 11], 7: [1, 2], 2: [4, 5, 6, 8]})
    assert model.hub_set(a) == [0, 2, 3, 5]
    assert list(model.union_rows(a, [0, 2, 3, 5])) == list(range(1, 12))
    assert list(model.union_rows(a, [5, 3])) == [1, 2, 3, 9, 10, 11]


def test_at_most_32_hubs_the_smaller_id_on_a_tie():
    out = {0: range(40, 80)}
    for h in range(1, 35):
        out[h] = range(40, 40 + (12 if h % 2 else 11))           # 17 rows of 12 entries, 17 of 11: all at or above the quarter (10)
    hubs = model.hub_set(graph(80, out))
    assert len(hubs) == 32 and hubs[0] == 0
    assert hubs[1:18] == list(range(1, 35, 2)) and hubs[18:] == list(range(2, 30, 2))


def test_levels_follow_the_two_shares():
    # 0 -> 1 .. 8; rows 1 .. 8 hold 8 + 8 entries (from 0 and from 20), rows 9 .. 12 hold what 10 and 11 give them
    base = {0: range(1, 9), 20: range(1, 9), 21: [22]}
    assert model.hub_set(graph(24, base)) == [0, 20]
    assert model.levels(graph(24, base)) == 1                    # two hubs with the same out-rows: no extra rows
    assert model.levels(graph(24, {0: range(1, 9), 20: range(1, 9)})) == 0   # nothing would be left
    two = {**base, 10: [9, 10, 11, 12], 11: [9, 10, 11, 12], 13: [9], 14: [9]}
    a = graph(24, two)
    assert model.hub_set(a) == [0, 20, 10, 11]
    first, extra = model.shares(a, model.hub_set(a))
    assert (first, extra) == (16 / 27, 10 / 27) and model.levels(a) == 2
    thin = {**base, 10: [9, 1], 11: [9, 2]}               # extra row 9 holds 2 of 21 entries: under an eighth
    assert model.hub_set(graph(24, thin)) == [0, 20, 10, 11] and model.levels(graph(24, thin)) == 1
    flat = {u: [(u + 1) % 24, (u + 2) % 24] for u in range(24)}  # no row holds a quarter of the entries
    assert model.levels(graph(24, flat)) == 0


def test_tiers_and_the_cut_of_a_whole_frontier_call():
    """Hubs 0 and 1.  t_a = 2 -> both, t_b = 3 -> hub 0 only.  Sources 10 .. 15 -> t_a and another vertex (tier A), 16 .. 18 -> t_b
    and another (tier B), 19 .. 21 weak, 22 dead; passes of 2 rows."""
    out = {0: range(30, 50), 1: range(40, 60), 2: [0, 1], 3: [0]}
    for s in range(10, 16):
        out[s] = [2, 25]
    for s in range(16, 19):
        out[s] = [3, 25]
    for s in range(19, 22):
        out[s] = [25, 26]
    a = graph(60, out)
    at = oracle.transpose(a)
    assert model.hub_set(a) == [0, 1]
    src = np.array([19, 10, 16, 22, 11, 20, 12, 17, 13, 14, 21, 15, 18], dtype=U64)
    assert list(model.tiers(a, at, src, [0, 1])) == [0, 2, 1, 0, 2, 0, 2, 1, 2, 2, 0, 2, 1]
    assert list(model.tiers(a, at, src, [0])) == [0, 2, 2, 0, 2, 0, 2, 2, 2, 2, 0, 2, 2]
    # 12 live rows, A x 6, B x 3, weak x 3: passes AA AA AA BB Bw ww
    assert model.tiered_passes(a, at, src, 2) == (6, 4, 3, 0, 12)
    assert model.tiered_passes(a, at, src, 2, hubs=[0]) == (6, 4, 4, 0, 12)
    assert model.tiered_passes(a, at, src, 4) == (3, 2, 1, 0, 12)   # AAAA AABB Bwww


def test_degree_one_classes_keep_their_tier():
    """Four degree-one sources on the tier-A target 2, four on the weak target 25; two plain tier-A sources; passes of 1 row.
    Classes of four: kmax = 2 gives one row of scale four each."""
    out = {0: range(30, 50), 1: range(40, 60), 2: [0, 1], 25: [26]}
    for s in range(10, 14):
        out[s] = [2]
    for s in range(14, 18):
        out[s] = [25]
    out[18] = [2, 26]
    out[19] = [2, 26]
    a = graph(60, out)
    at = oracle.transpose(a)
    src = np.arange(10, 20, dtype=U64)
    total, strong, deep, deep_scaled, live = model.tiered_passes(a, at, src, 1)
    assert (total, strong, deep, deep_scaled, live) == (4, 3, 3, 1, 10)
