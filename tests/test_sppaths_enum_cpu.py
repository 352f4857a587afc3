"""CPU: the checker of tests/sppaths_enum_check.py (what the GPU tests hold fgpu_sssp_hops, algo_sp_paths_rows and algo_ss_paths
to) against the reference's own graphs and asserted results (tests/golden/sppaths_enum_flow.json), its pruned walk against its
unpruned one on the seeded cases, and the D_h recurrence on cases worked by hand."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sppaths_enum_check as K  # noqa: E402
from msf_check import bits_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "sppaths_enum_flow.json")))
INF = float("inf")


def golden_graph(case):
    """(n, edges [(id, type, src, dst)], type names in creation order, node id by name, attributes by relationship id)"""
    if "branchy" in case:
        b = FLOW["branchy"][case["branchy"]]
        at = {v: (v - 1 if v else b["blob"]) for v in range(b["blob"] + 1)}
        edges = [(i, b["type"], i // b["fanout"], y - 1) for i, y in enumerate(b["dst"])]
        return b["blob"] + 1, edges, [b["type"]], at, {}
    at = {name: k for k, (name, _) in enumerate(case["nodes"])}
    edges, order = [], []
    for i, (a, t, b, _) in enumerate(case["edges"]):
        edges.append((i, t, at[a], at[b]))
        if t not in order:
            order.append(t)
    return max(len(at), 1), edges, order, at, {i: e[3] for i, e in enumerate(case["edges"])}


def golden_call(case):
    """the arguments of K.paths for the case's call"""
    n, edges, order, at, attrs = golden_graph(case)
    c = case["call"]
    prop = lambda name: None if name is None else {i: a[name] for i, a in attrs.items() if name in a}
    kw = {"types": c["types"], "direction": c["direction"], "max_len": c["max_len"], "max_cost": c["max_cost"],
          "path_count": c["path_count"], "weights": prop(c["weight"]), "costs": prop(c["cost"])}
    return (edges, order, n, at[c["source"]], None if c["target"] is None else at[c["target"]]), kw


def expect(case, rows):
    exp = case["call"]["expect"]
    assert len(rows) == exp["rows"]
    if "weights_desc" in exp:
        got = sorted((r[2] for r in rows), reverse=True)
        assert all(abs(g - w) <= exp["delta"] for g, w in zip(got, exp["weights_desc"])), got
    if "lengths_sorted" in exp:
        assert sorted(len(r[0]) for r in rows) == exp["lengths_sorted"]


@pytest.mark.parametrize("case", FLOW["cases"], ids=lambda c: c["name"])
def test_checker_gives_what_the_reference_asserts(case):
    args, kw = golden_call(case)
    # the 3000-node graph is walked pruned only: its unpruned walks take 37 000 to 294 000 steps (a minute in Python)
    deep = case.get("branchy") == "3000x8"
    pruned = K.paths(*args, prune=True, **kw)
    expect(case, pruned)
    if not deep or case["call"]["max_len"] <= 5:
        assert K.paths(*args, prune=False, **kw) == pruned


def test_deep_search_counts():
    case = next(c for c in FLOW["cases"] if c["name"] == "10_deep_7_88_maxLen_5_pathCount_0")
    args, kw = golden_call(case)
    a, b = {}, {}
    assert K.paths(*args, prune=False, stats=a, **kw) == K.paths(*args, prune=True, stats=b, **kw)
    assert (a["examined"], b["examined"], b["table_rows"]) == (37024, 56, 6)
    case = next(c for c in FLOW["cases"] if c["name"] == "10_deep_1_137_maxLen_5_pathCount_0")
    args, kw = golden_call(case)
    assert K.paths(*args, prune=True, stats=b, **kw) == [] and b["examined"] == 0


@pytest.mark.parametrize("seed", K.SEEDS)
def test_pruned_walk_equals_unpruned_walk(seed):
    n, edges, weights, costs = K.seeded_graph(seed)
    for source, target, kw in K.seeded_calls(seed):
        a, b = {}, {}
        plain = K.paths(edges, ["R", "S"], n, source, target, weights=weights, costs=costs, prune=False, stats=a, **kw)
        pruned = K.paths(edges, ["R", "S"], n, source, target, weights=weights, costs=costs, prune=True, stats=b, **kw)
        assert plain == pruned, (source, target, kw)
        assert b["examined"] <= a["examined"]
        for e, nodes, w, c in plain:   # a simple walk over the relationships, in the right direction
            assert nodes[0] == source and nodes[-1] == target and len(set(nodes)) == len(nodes) == len(e) + 1


def test_the_sweep_covers_every_value_of_every_axis():
    seen = {k: set() for k in ("types", "direction", "max_len", "max_cost", "path_count")}
    informative = 0
    for seed in K.SEEDS:
        n, edges, weights, costs = K.seeded_graph(seed)
        for source, target, kw in K.seeded_calls(seed):
            for k in seen:
                seen[k].add(kw[k])
            informative += len(K.paths(edges, ["R", "S"], n, source, target, weights=weights, costs=costs, **kw)) > 1
    assert seen["types"] == set(K.REL_TYPES) and seen["direction"] == set(K.DIRECTIONS) and seen["max_len"] == set(K.MAX_LENS)
    assert seen["max_cost"] == set(K.MAX_COSTS) and seen["path_count"] == set(K.PATH_COUNTS)
    assert informative >= 25   # calls that return several rows: the order of the rows is under test too


@pytest.mark.parametrize("max_len", [32, 33, 34, 35, 36, None])
@pytest.mark.parametrize("path_count", [0, 1, 2])
def test_hop_limited_optimum_heavier_than_the_unbounded_one(max_len, path_count):
    # beyond 32 hops the table is fgpu_sssp's one row, which knows no hop budget: it must not seed the bound (35.0) below the
    # only path that qualifies under maxLen 33 or 34 (100.0)
    n, edges, weights = K.detour_graph()
    st = {}
    plain = K.paths(edges, ["R"], n, 0, n - 1, weights=weights, max_len=max_len, path_count=path_count, prune=False)
    pruned = K.paths(edges, ["R"], n, 0, n - 1, weights=weights, max_len=max_len, path_count=path_count, prune=True, stats=st)
    assert plain == pruned and st["table_rows"] == (33 if max_len == 32 else 0)
    short = max_len is not None and max_len < 35
    if short:
        assert [r[2] for r in plain] == [100.0]
    else:
        assert [r[2] for r in plain] == ([35.0, 100.0] if path_count == 2 else [35.0])
    # a target out of reach within maxLen, in reach without: no rows, and no walk
    far = K.paths(edges[:-1], ["R"], n, 0, n - 1, weights=weights, max_len=33 if max_len is None else min(max_len, 34),
                  path_count=path_count, prune=True, stats=st)
    assert far == [] and st["examined"] == 0


def test_k_list_keeps_new_paths_in_front_of_their_equals():
    # three parallel routes 0 -> k -> 4 of equal weight, cost and length: pathCount 2 keeps the LAST two the walk finds, the
    # later one first (partition_point puts a path in front of its equals; an equal candidate never replaces a kept one)
    edges = [(0, "R", 0, 1), (1, "R", 0, 2), (2, "R", 0, 3), (3, "R", 1, 4), (4, "R", 2, 4), (5, "R", 3, 4)]
    rows = K.paths(edges, ["R"], 5, 0, 4, path_count=2, max_len=3)
    assert [r[0] for r in rows] == [[1, 4], [2, 5]]   # found in the order [2, 5], [1, 4], [0, 3] (popped from the back)
    assert [r[0] for r in K.paths(edges, ["R"], 5, 0, 4, path_count=0, max_len=3)] == [[2, 5], [1, 4], [0, 3]]
    assert [r[0] for r in K.paths(edges, ["R"], 5, 0, 4, path_count=1, max_len=3)] == [[2, 5]]
    # a type listed twice hands every successor out twice: every path comes twice
    assert len(K.paths(edges, ["R"], 5, 0, 4, types=["R", "R"], path_count=0, max_len=3)) == 12
    with pytest.raises(ValueError):
        K.paths(edges, ["R"], 5, 0, 4, path_count=-1)
    with pytest.raises(ValueError):
        K.paths(edges, ["R"], 5, 0, 4, weights={1: -0.5}, max_len=3)
    with pytest.raises(RuntimeError):
        K.paths(edges, ["R"], 5, 0, 4, path_count=0, max_len=3, max_examined=4)


def test_hop_table_by_hand():
    t, st = K.hop_table(4, [0, 1, 2, 0], [1, 2, 3, 3], bits_of([1.0, 1.0, 1.0, 10.0]), 0, 5)
    assert list(t[:, 3]) == [INF, 10.0, 10.0, 3.0, 3.0, 3.0] and st == [4, 5, 4, 4]   # frontiers {0}, {1, 3}, {2}, {3}, {}
    t, st = K.hop_table(3, [0, 1], [1, 2], None, 0, 0)
    assert t.shape == (1, 3) and st == [0, 0, 0, 1]
    # 0.1 + 0.2 + 0.3 from the far end is not the walk's fold: the slack of the pruning rule exists for this
    back, _ = K.hop_table(4, [3, 2, 1], [2, 1, 0], bits_of([0.3, 0.2, 0.1]), 3, 3)
    assert back[3, 0] == 0.3 + 0.2 + 0.1 != 0.1 + 0.2 + 0.3
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError):
            K.hop_table(2, [0], [1], bits_of([bad]), 0, 1)
