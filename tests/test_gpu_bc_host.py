"""GPU: algo.betweenness through the host layer (fh_algo_betweenness, algo_procedures.rs:884-1017) — the reference's flow
cases (tests/golden/betweenness_flow.json, from its tests/flow/test_betweenness.py), label-filtered runs whose sources are
compact indices, deleted nodes, and a random host graph against the numpy checker of tests/bc_check.py."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bc_check import betweenness, csr_of  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "betweenness_flow.json")))["cases"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node with id k is node index k - 1"""
    n = len(case["nodes"])
    g = host.Graph(hctx, max(n, 1))
    if n == 0:
        g.delete_node(0)
    labels, types = {}, {}
    for nd in case["nodes"]:
        for l in nd["labels"]:
            if l not in labels:
                labels[l] = g.add_label(l)
            g.label_node(nd["id"] - 1, labels[l])
    for eid, (a, t, b) in enumerate(case["edges"]):
        if t not in types:
            types[t] = g.add_type(t)
        g.create_edge(types[t], a - 1, b - 1, eid)
    return g


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))).all(), (got, want)


def scores_by_name(case, q, g):
    nodes, scores = g.algo_betweenness(q["labels"], q["types"], q["samplingSize"], q["samplingSeed"])
    assert nodes.tolist() == sorted(nodes.tolist())
    names = {nd["id"] - 1: nd["name"] for nd in case["nodes"]}
    return {names[int(v)]: float(s) for v, s in zip(nodes, scores)}


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g = build(hctx, case)
    got = []
    for q in case["queries"]:
        s = scores_by_name(case, q, g)
        assert sorted(s) == sorted(q["scores"]), q
        close([s[k] for k in sorted(s)], [q["scores"][k] for k in sorted(s)])
        for op, a, b in q["relations"]:
            rhs = s[b] if isinstance(b, str) else b
            assert (s[a] > rhs) if op == ">" else (s[a] == rhs), (op, a, b, s)
        got.append(s)
    if case["name"] == "relationship_types":
        assert got[0]["B"] != got[1]["B"]
    if case["name"] == "combined_parameters":
        assert all(got[1][x] == got[2][x] for x in "ABC")             # Person + FRIEND == FRIEND on the Person nodes
        assert got[1]["B"] != got[5]["B"]
        assert got[6]["B"] != got[7]["B"]                               # different seeds, different samples


def test_invalid_sampling_size_and_empty_selections(hctx):
    case = next(c for c in FLOW if c["name"] == "betweenness_centrality")
    g = build(hctx, case)
    for bad in (0, -21):
        with pytest.raises(host.HostError) as e:
            g.algo_betweenness(sampling_size=bad)
        assert "samplingSize must be a positive integer" in str(e.value)
    assert len(g.algo_betweenness(["Nope"])[0]) == 0                     # labels that select nothing
    nodes, scores = g.algo_betweenness([], ["Nope"])                      # unknown types add no edges
    assert nodes.tolist() == list(range(5)) and scores.tolist() == [0.0] * 5
    nodes, scores = g.algo_betweenness(sampling_size=(1 << 32) + 1)      # 2^32 + 1 means one source: index 0 (A)
    assert scores.tolist() == [0.0, 3.0, 0.5, 0.5, 0.0]
    nodes, scores = g.algo_betweenness(sampling_size=1 << 31)            # 2^31: every node
    assert scores.tolist() == [0.0, 3.0, 1.0, 1.0, 0.0]


def test_label_filtered_sources_are_compact_indices(hctx):
    # a path 0 -> 1 -> 2 -> 3 -> 4 -> 5; label L on {1, 3, 4, 5}: the induced subgraph is 3 -> 4 -> 5 plus an isolated 1.
    # samplingSize 2, seed 0: compact indices 0 and 1 = nodes 1 and 3 — node 3 puts 1 on node 4
    g = host.Graph(hctx, 6)
    lab = g.add_label("L")
    t = g.add_type("R")
    for v in (1, 3, 4, 5):
        g.label_node(v, lab)
    for v in range(5):
        g.create_edge(t, v, v + 1, v)
    nodes, scores = g.algo_betweenness(["L"], [], 2, 0)
    assert nodes.tolist() == [1, 3, 4, 5] and scores.tolist() == [0.0, 0.0, 1.0, 0.0]
    nodes, scores = g.algo_betweenness(["L"], [], 1, 0)                  # compact index 0 = node 1: reaches nothing
    assert scores.tolist() == [0.0] * 4
    nodes, scores = g.algo_betweenness([], [], 2, 0)                      # unfiltered: ids 0 and 1
    assert nodes.tolist() == list(range(6)) and scores.tolist() == [0.0, 4.0, 6.0, 4.0, 2.0, 0.0]


def test_deleted_nodes(hctx):
    # a path 0 -> 1 -> 2 -> 3; node 1 deleted (its edges stay in the matrix, as in the reference): it is still a vertex and
    # can be a source, but leaves the output
    g = host.Graph(hctx, 4)
    t = g.add_type("R")
    for v in range(3):
        g.create_edge(t, v, v + 1, v)
    g.delete_node(1)
    nodes, scores = g.algo_betweenness(sampling_size=2, sampling_seed=0)   # n_nodes = 3 live + 1 deleted: sources 0, 1
    assert nodes.tolist() == [0, 2, 3] and scores.tolist() == [0.0, 2.0, 0.0]
    g.delete_node(0)
    g.delete_node(2)
    g.delete_node(3)
    assert len(g.algo_betweenness()[0]) == 0                              # no live node: an empty result


@pytest.mark.parametrize("seed", [0, 1])
def test_random_host_graph_matches_the_checker(hctx, seed):
    rng = np.random.default_rng(seed)
    n = 2000
    g = host.Graph(hctx, n)
    lab = {name: g.add_label(name) for name in ("P", "Q")}
    typ = {name: g.add_type(name) for name in ("A", "B")}
    has = {name: rng.random(n) < p for name, p in (("P", 0.6), ("Q", 0.3))}
    for name, m in has.items():
        for v in np.flatnonzero(m):
            g.label_node(int(v), lab[name])
    doomed = rng.choice(n, 40, replace=False)
    free = np.setdiff1d(np.arange(n), doomed)
    edges = []
    for eid in range(8000):
        t = ("A", "B")[int(rng.integers(0, 2))]
        a, b = (int(x) for x in rng.choice(free, 2))
        edges.append((t, a, b))
        g.create_edge(typ[t], a, b, eid)
    for v in doomed:
        g.delete_node(int(v))
    live = np.ones(n, dtype=bool)
    live[doomed] = False
    for labels, types, size, sd in [((), (), 16, 0), ((), ("A",), 40, 7), (("P",), (), 16, -3), (("P", "Q"), ("B",), 25, 0)]:
        sel = [e for e in edges if not types or e[0] in types]
        rp, ci = csr_of(n, [e[1] for e in sel], [e[2] for e in sel])
        if labels:
            active = np.zeros(n, dtype=bool)
            for name in labels:
                active |= has[name]
            active &= live
            ids = np.flatnonzero(active)
            src = ids[host.betweenness_sources(len(ids), size, sd).astype(np.int64)]
        else:
            active = None
            src = host.betweenness_sources(n, size, sd).astype(np.int64)
        want = betweenness(n, rp, ci, src, active)[0]
        nodes, scores = g.algo_betweenness(list(labels), list(types), size, sd)
        keep = live if active is None else active
        assert nodes.tolist() == np.flatnonzero(keep).tolist()
        close(scores, want[keep])
