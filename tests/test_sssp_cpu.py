"""CPU: the checker of tests/sssp_check.py (what the GPU tests hold fgpu_sssp to) against the reference's own graphs and expected
weights (tests/golden/sppaths_flow.json), against an independent Bellman-Ford with bitwise-equal distances, and for the validity
of the parent tree its rule produces."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of  # noqa: E402
from sssp_check import sssp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "sppaths_flow.json")))["cases"]
U64 = np.uint64
# the weights of the experiment behind the rules of include/fgpu.h: zeros, weights that are absorbed, weights that overflow
WEIGHTS = np.array([0.0, 1e-20, 1e-17, 0.1, 0.2, 0.3, 1.0, 2.0, 3.5, 1e300])


def entries_of(case):
    """the directed weighted entries of a case's graph the way the procedure sees them for an outgoing search over weightProp:
    self-loops dropped, the cheapest relationship per ordered pair"""
    at = {name: k for k, (name, _) in enumerate(case["nodes"])}
    prop = case["config"]["weight"]
    best = {}
    for a, _, b, attrs in case["edges"]:
        if a == b:
            continue
        w = float(attrs.get(prop, 1.0)) if prop else 1.0
        key = (at[a], at[b])
        best[key] = min(best.get(key, w), w)
    rows = [k[0] for k in best]
    cols = [k[1] for k in best]
    return at, len(case["nodes"]), rows, cols, bits_of(list(best.values()))


@pytest.mark.parametrize("case", [c for c in FLOW if "pairs" in c["expect"]], ids=lambda c: c["name"])
def test_reference_graphs_every_ordered_pair(case):
    at, n, rows, cols, bits = entries_of(case)
    dist = {s: sssp(n, rows, cols, bits, s)[0] for s in range(n)}
    for s, t, want in case["expect"]["pairs"]:
        got = dist[s][t]
        if want is None:
            assert np.isinf(got), (s, t)
        else:
            assert abs(got - want) <= case["expect"]["delta"], (s, t, got, want)


@pytest.mark.parametrize("case", [c for c in FLOW if "pairs" not in c["expect"] and c["config"]["direction"] == "outgoing"],
                         ids=lambda c: c["name"])
def test_reference_single_calls(case):
    at, n, rows, cols, bits = entries_of(case)
    cfg, exp = case["config"], case["expect"]
    dist, parent, depth = sssp(n, rows, cols, bits, at[cfg["source"]])
    t = at[cfg["target"]]
    assert np.isfinite(dist[t]) == exp["found"]
    if not exp["found"]:
        return
    path = [t]
    while path[-1] != at[cfg["source"]]:
        path.append(int(parent[path[-1]]))
    names = [case["nodes"][v][0] for v in reversed(path)]
    if "nodes" in exp:
        assert names == exp["nodes"]
    if "hops" in exp:
        assert len(path) - 1 == exp["hops"]
    if "weight" in exp:
        assert abs(dist[t] - exp["weight"]) <= exp["delta"]


def bellman_ford(n, rows, cols, w, src, rng):
    """label-correcting over the entries in a shuffled order until nothing changes: a different algorithm, the same fixed point"""
    dist = np.full(n, np.inf)
    dist[src] = 0.0
    order = rng.permutation(len(rows))
    for _ in range(n + 1):
        changed = False
        for k in order:
            u, v = rows[k], cols[k]
            nd = dist[u] + w[k]
            if u != v and np.isfinite(nd) and nd < dist[v]:
                dist[v] = nd
                changed = True
        if not changed:
            return dist
    raise AssertionError("no fixed point")


def random_graph(rng, n, m):
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    key = np.unique(a * n + b)   # distinct ordered pairs; the diagonal stays in (it must be ignored)
    return key // n, key % n


@pytest.mark.parametrize("seed", range(40))
def test_dijkstra_equals_bellman_ford_bit_for_bit(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 40))
    rows, cols = random_graph(rng, n, int(rng.integers(1, 5 * n)))
    w = rng.choice(WEIGHTS, len(rows))
    src = int(rng.integers(0, n))
    dist, parent, depth = sssp(n, rows, cols, bits_of(w), src)
    want = bellman_ford(n, rows, cols, w, src, rng)
    assert np.array_equal(dist.view(U64), want.view(U64))
    check_tree(n, rows, cols, w, src, dist, parent, depth)


def check_tree(n, rows, cols, w, src, dist, parent, depth):
    """every chain ends at src within depth[v] steps, every parent entry is tight, and the parent is the smallest qualifying one"""
    weight = {(int(u), int(v)): float(x) for u, v, x in zip(rows, cols, w)}
    assert parent[src] == src and depth[src] == 0
    for v in range(n):
        if not np.isfinite(dist[v]):
            assert parent[v] == -1 and depth[v] == -1
            continue
        x = v
        for _ in range(int(depth[v])):
            u = int(parent[x])
            assert u != x and dist[u] + weight[(u, x)] == dist[x] and depth[u] + 1 == depth[x]
            smaller = [p for p in range(u) if (p, x) in weight and p != x and np.isfinite(dist[p])
                       and dist[p] + weight[(p, x)] == dist[x] and depth[p] + 1 == depth[x]]
            assert not smaller
            x = u
        assert x == src


def test_zero_weight_cycles_and_absorbed_weights_give_a_tree():
    # the graphs on which "the tight in-neighbour with the smallest (dist, id)" runs in circles
    rows = np.array([0, 1, 2, 0, 3, 4, 5, 5])
    cols = np.array([1, 2, 1, 3, 4, 5, 3, 6])
    w = np.array([1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0])
    dist, parent, depth = sssp(7, rows, cols, bits_of(w), 0)
    check_tree(7, rows, cols, w, 0, dist, parent, depth)
    assert list(parent) == [0, 0, 1, 0, 3, 4, 5] and list(depth) == [0, 1, 2, 1, 2, 3, 4]
    rows = np.array([0, 0, 1, 2, 2, 3, 1])
    cols = np.array([1, 2, 2, 1, 3, 2, 3])
    w = np.array([1.0, 1.0, 1e-20, 1e-20, 1.0, 1e-20, -0.0])
    dist, parent, depth = sssp(4, rows, cols, bits_of(w), 0)
    check_tree(4, rows, cols, w + 0.0, 0, dist, parent, depth)
    assert list(dist) == [0.0, 1.0, 1.0, 1.0] and list(parent) == [0, 0, 0, 1]


def test_rejects_nan_and_negative_weights():
    for bad in (float("nan"), -1.0, -float("inf")):
        with pytest.raises(ValueError):
            sssp(2, [0], [1], bits_of([bad]), 0)
    dist, parent, _ = sssp(3, [0, 1], [1, 2], bits_of([1.0, float("inf")]), 0)
    assert np.isinf(dist[2]) and parent[2] == -1
    dist, _, depth = sssp(3, [0, 1], [1, 2], None, 0)   # a BOOL matrix: every weight 1.0
    assert list(dist) == [0.0, 1.0, 2.0] and list(depth) == [0, 1, 2]
