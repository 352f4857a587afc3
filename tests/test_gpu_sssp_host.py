"""GPU: algo.SPpaths' single cheapest path through the host layer (fh_algo_sp_paths; run_path_algo's Dijkstra branch,
algo_procedures.rs:2548-2597) — what the reference's flow tests assert (tests/golden/sppaths_flow.json, from its
tests/flow/test_path_algorithms.py: tests 12, 13, 16, 17a and 19 to 22), then what those graphs do not reach: multi-edges,
unlisted relationships, a self-loop at source == target, negative weights, and a random multigraph against the checker of
tests/sssp_check.py run on the pair reduction restated in numpy.  Every returned path is walked."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of  # noqa: E402
from sssp_check import sssp  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "sppaths_flow.json")))["cases"]
U64 = np.uint64


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node k of the case is node id k, edge k relationship id k"""
    n = len(case["nodes"])
    g = host.Graph(hctx, max(n, 1))
    at, labels, types = {}, {}, {}
    for k, (name, label) in enumerate(case["nodes"]):
        at[name] = k
        if label is not None:
            if label not in labels:
                labels[label] = g.add_label(label)
            g.label_node(k, labels[label])
    for eid, (a, t, b, _) in enumerate(case["edges"]):
        if t not in types:
            types[t] = g.add_type(t)
        g.create_edge(types[t], at[a], at[b], eid)
    return g, at


def attribute(case, prop):
    if prop is None:
        return None
    return {eid: e[3][prop] for eid, e in enumerate(case["edges"]) if prop in e[3]}


def walk(edges, direction, weights, got, source, target):
    """the returned path is a walk over the returned relationships in the requested direction whose weights fold to `weight`,
    bit for bit; edges: {relationship id: (src, dst)}"""
    nodes, rels, weight, cost = got
    assert nodes[0] == source and nodes[-1] == target and len(rels) == len(nodes) - 1
    total = 0.0
    for k, e in enumerate(rels):
        a, b = edges[int(e)]
        step = (int(nodes[k]), int(nodes[k + 1]))
        ways = {"outgoing": [(a, b)], "incoming": [(b, a)], "both": [(a, b), (b, a)]}[direction]
        assert step in ways, (step, e)
        total = total + (1.0 if weights is None else float(weights.get(int(e), 1.0)))
    assert np.float64(total).view(U64) == np.float64(weight).view(U64)


@pytest.mark.parametrize("case", [c for c in FLOW if "pairs" not in c["expect"]], ids=lambda c: c["name"])
def test_reference_single_calls(hctx, case):
    g, at = build(hctx, case)
    cfg, exp = case["config"], case["expect"]
    weights, costs = attribute(case, cfg["weight"]), attribute(case, cfg["cost"])
    got = g.algo_sp_paths(at[cfg["source"]], at[cfg["target"]], cfg["types"], cfg["direction"], weights, costs)
    assert (got is not None) == exp["found"]
    if got is None:
        return
    nodes, rels, weight, cost = got
    edges = {eid: (at[a], at[b]) for eid, (a, _, b, _) in enumerate(case["edges"])}
    walk(edges, cfg["direction"], weights, got, at[cfg["source"]], at[cfg["target"]])
    if "nodes" in exp:
        assert [case["nodes"][int(v)][0] for v in nodes] == exp["nodes"]
    if "hops" in exp:
        assert len(rels) == exp["hops"]
    if "weight" in exp:
        assert abs(weight - exp["weight"]) <= exp["delta"]
    if "cost" in exp:
        assert cost == exp["cost"]


@pytest.mark.parametrize("case", [c for c in FLOW if "pairs" in c["expect"]], ids=lambda c: c["name"])
def test_reference_graphs_every_ordered_pair(hctx, case):
    g, at = build(hctx, case)
    cfg, exp = case["config"], case["expect"]
    weights = attribute(case, cfg["weight"])
    edges = {eid: (at[a], at[b]) for eid, (a, _, b, _) in enumerate(case["edges"])}
    for s, t, want in exp["pairs"]:
        got = g.algo_sp_paths(s, t, cfg["types"], cfg["direction"], weights)
        if want is None:
            assert got is None, (s, t)
        else:
            assert got is not None and abs(got[2] - want) <= exp["delta"], (s, t, got, want)
            walk(edges, cfg["direction"], weights, got, s, t)


def small(hctx, n, edges, types=("R",)):
    """edges: (src, dst) or (src, dst, type index); relationship id = position"""
    g = host.Graph(hctx, n)
    tids = [g.add_type(t) for t in types]
    for eid, e in enumerate(edges):
        g.create_edge(tids[e[2] if len(e) > 2 else 0], e[0], e[1], eid)
    return g


def test_multi_edges_keep_the_cheapest_then_the_smallest_id(hctx):
    g = small(hctx, 3, [(0, 1), (0, 1), (0, 1), (1, 2), (1, 2)])
    nodes, rels, weight, cost = g.algo_sp_paths(0, 2, weights={0: 5.0, 1: 2.0, 2: 2.0, 3: 1.0, 4: 1.0}, costs={1: 7.0, 2: 100.0, 3: 0.5})
    assert list(nodes) == [0, 1, 2] and list(rels) == [1, 3] and weight == 3.0 and cost == 7.5
    # across types as well, and a type listed twice or unknown changes nothing
    g = small(hctx, 2, [(0, 1, 0), (0, 1, 1)], types=("R", "S"))
    w = {0: 4.0, 1: 3.0}
    assert list(g.algo_sp_paths(0, 1, weights=w)[1]) == [1]
    assert list(g.algo_sp_paths(0, 1, types=["R", "R", "nope"], weights=w)[1]) == [0]
    assert g.algo_sp_paths(0, 1, types=["nope"], weights=w) is None


def test_unlisted_relationship_weighs_one_and_costs_nothing(hctx):
    g = small(hctx, 3, [(0, 1), (1, 2), (0, 2)])
    nodes, rels, weight, cost = g.algo_sp_paths(0, 2, weights={2: 2.5}, costs={2: 9.0})
    assert list(rels) == [0, 1] and weight == 2.0 and cost == 0.0
    nodes, rels, weight, cost = g.algo_sp_paths(0, 2, weights={2: 1.5}, costs={2: 9.0})
    assert list(rels) == [2] and weight == 1.5 and cost == 9.0
    # a weight that is no finite number takes the relationship out; with it the only route goes
    assert list(g.algo_sp_paths(0, 2, weights={2: float("inf")})[1]) == [0, 1]
    assert g.algo_sp_paths(0, 2, weights={2: float("nan"), 0: float("inf")}) is None


def test_source_equals_target_is_not_found(hctx):
    g = small(hctx, 2, [(0, 0), (0, 1), (1, 0)])
    assert g.algo_sp_paths(0, 0) is None
    assert g.algo_sp_paths(0, 0, direction="both", weights={0: 1.0}) is None
    assert g.algo_sp_paths(0, 7) is None and g.algo_sp_paths(9, 1) is None   # out of range
    g.delete_node(1)
    assert g.algo_sp_paths(0, 1) is None


def test_negative_weight_raises_and_names_the_relationship(hctx):
    g = small(hctx, 3, [(0, 1), (1, 2)])
    with pytest.raises(host.HostError) as e:
        g.algo_sp_paths(0, 2, weights={1: -0.5})
    assert "negative weight" in str(e.value) and "relationship 1" in str(e.value)
    assert g.algo_sp_paths(0, 2, weights={1: -0.0})[2] == 1.0   # -0.0 is 0.0
    assert list(g.algo_sp_paths(0, 2, weights={1: 0.5})[1]) == [0, 1]   # the graph still answers


@pytest.mark.parametrize("direction", ["outgoing", "incoming", "both"])
def test_random_multigraph_against_the_checker(hctx, direction):
    rng = np.random.default_rng(0x5B9A)
    n, m = 200, 900
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)   # self-loops and multi-edges included
    typ = rng.integers(0, 2, m)
    w = rng.integers(1, 9, m).astype(np.float64) / 4.0
    g = small(hctx, n, list(zip(src.tolist(), dst.tolist(), typ.tolist())), types=("R", "S"))
    listed = {k: float(w[k]) for k in range(m) if k % 7}          # every seventh relationship is unlisted: 1.0
    eff = np.array([listed.get(k, 1.0) for k in range(m)])
    # the pair reduction: per ordered pair in traversal direction the smallest (weight, id)
    a = {"outgoing": src, "incoming": dst, "both": np.concatenate([src, dst])}[direction]
    b = {"outgoing": dst, "incoming": src, "both": np.concatenate([dst, src])}[direction]
    ids = np.arange(m) if direction != "both" else np.concatenate([np.arange(m), np.arange(m)])
    ww = eff[ids]
    keep = a != b
    a, b, ids, ww = a[keep], b[keep], ids[keep], ww[keep]
    order = np.lexsort((ids, ww, b, a))
    a, b, ids, ww = a[order], b[order], ids[order], ww[order]
    first = np.concatenate([[True], (a[1:] != a[:-1]) | (b[1:] != b[:-1])])
    a, b, ids, ww = a[first], b[first], ids[first], ww[first]
    rel = {(int(x), int(y)): int(k) for x, y, k in zip(a, b, ids)}
    edges = {k: (int(src[k]), int(dst[k])) for k in range(m)}
    for s in (0, 17, 101):
        dist, parent, _ = sssp(n, a, b, bits_of(ww), s)
        for t in range(0, n, 3):
            got = g.algo_sp_paths(s, t, direction=direction, weights=listed)
            if t == s or not np.isfinite(dist[t]):
                assert got is None
                continue
            nodes, rels, weight, cost = got
            assert np.float64(weight).view(U64) == dist[t].view(U64)
            chain = [t]
            while chain[-1] != s:
                chain.append(int(parent[chain[-1]]))
            assert list(nodes) == chain[::-1]
            assert list(rels) == [rel[(chain[k + 1], chain[k])] for k in range(len(chain) - 1)][::-1]
            walk(edges, direction, listed, got, s, t)
