"""GPU: algo.labelPropagation through the host layer (fh_algo_cdlp, algo_procedures.rs:1168-1270) — the reference's flow
cases (tests/golden/cdlp_flow.json, from its tests/flow/test_cdlp.py), the compact communityIds of a label-filtered run,
deleted nodes, the maxIterations rule, and a random host graph against the numpy checker of tests/cdlp_check.py."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdlp_check import cdlp_labels, csr_of  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "cdlp_flow.json")))["cases"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node with id = k is node index k - 1"""
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


def grouped(nodes, comm, id_of=lambda v: int(v) + 1):
    by = {}
    for v, c in zip(nodes.tolist(), comm.tolist()):
        by.setdefault(c, []).append(id_of(v))
    return sorted((sorted(x) for x in by.values()), key=lambda x: (len(x), x))


def sym_csr(n, edges):
    a, b = [e[1] for e in edges], [e[2] for e in edges]
    return csr_of(n, a + b, b + a)


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g = build(hctx, case)
    for q in case["queries"]:
        nodes, comm = g.algo_label_propagation(q["labels"], q["types"], q["max_iterations"])
        assert nodes.tolist() == sorted(nodes.tolist())
        assert grouped(nodes, comm) == q["communities"], q
        if q["max_iterations"] == 10:                                     # the procedure's default
            nodes2, comm2 = g.algo_label_propagation(q["labels"], q["types"])
            assert nodes2.tolist() == nodes.tolist() and comm2.tolist() == comm.tolist()


def test_empty_graph_gives_no_rows(hctx):
    g = build(hctx, {"nodes": [], "edges": []})
    nodes, comm = g.algo_label_propagation()
    assert len(nodes) == 0 and len(comm) == 0


def test_community_ids_unlabelled_are_node_ids_labelled_are_compact(hctx):
    case = next(c for c in FLOW if c["name"] == "node_label_filtering")
    g = build(hctx, case)
    # unlabelled: the label is a node id — every triangle ends on its smallest index
    nodes, comm = g.algo_label_propagation()
    assert nodes.tolist() == list(range(12)) and comm.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9]
    # User selects indices 6..11 -> ranks 0..5; the communityId is the winning label's rank
    nodes, comm = g.algo_label_propagation(["User"])
    assert nodes.tolist() == [6, 7, 8, 9, 10, 11] and comm.tolist() == [0, 0, 0, 3, 3, 3]
    nodes, comm = g.algo_label_propagation(["Person", "User"])              # the union of the labels: every node, rank = index
    assert nodes.tolist() == list(range(12)) and comm.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9]
    # unknown labels select nothing; an unknown label next to a known one adds nothing; unknown types add no edges
    assert len(g.algo_label_propagation(["Nope"])[0]) == 0
    assert g.algo_label_propagation(["Nope", "User"])[1].tolist() == [0, 0, 0, 3, 3, 3]
    nodes, comm = g.algo_label_propagation([], ["Nope"])
    assert nodes.tolist() == list(range(12)) and comm.tolist() == list(range(12))
    # one iteration: vertex 0 of a triangle takes the smaller neighbour, the others take 0
    nodes, comm = g.algo_label_propagation(["User"], [], 1)
    assert comm.tolist() == [1, 0, 0, 4, 3, 3]


def test_deleted_nodes_leave_the_output(hctx):
    case = next(c for c in FLOW if c["name"] == "basic")
    g = build(hctx, case)
    g.delete_node(8)
    nodes, comm = g.algo_label_propagation()
    assert nodes.tolist() == list(range(8))
    # (marked deleted; its edges stay in the matrix, as in the reference: 6 and 7 still hear its votes)
    assert comm.tolist() == [0, 0, 0, 3, 3, 3, 6, 6]
    for v in range(8):
        if v != 4:
            g.delete_node(v)
    nodes, comm = g.algo_label_propagation()
    assert nodes.tolist() == [4] and comm.tolist() == [3]
    g.delete_node(4)
    assert len(g.algo_label_propagation()[0]) == 0                         # no live node: an empty result


def test_max_iterations_must_be_positive(hctx):
    g = build(hctx, FLOW[0])
    for bad in (0, -21):
        with pytest.raises(host.HostError) as e:
            g.algo_label_propagation(max_iterations=bad)
        assert "maxIterations must be a positive integer" in str(e.value)
    empty = build(hctx, {"nodes": [], "edges": []})
    with pytest.raises(host.HostError):                                     # checked before the empty-graph exit
        empty.algo_label_propagation(max_iterations=0)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_host_graph_matches_the_checker(hctx, seed):
    rng = np.random.default_rng(seed)
    n = 3000
    g = host.Graph(hctx, n)
    lab = {name: g.add_label(name) for name in ("P", "Q", "R")}
    typ = {name: g.add_type(name) for name in ("A", "B", "C")}
    has = {name: rng.random(n) < p for name, p in (("P", 0.5), ("Q", 0.3), ("R", 0.1))}
    for name, m in has.items():
        for v in np.flatnonzero(m):
            g.label_node(int(v), lab[name])
    doomed = rng.choice(n, 60, replace=False)                 # deleted later: they get no edges
    free = np.setdiff1d(np.arange(n), doomed)
    edges = []                                                  # (type, src, dst, id) — repeats are multi-edges
    for eid in range(9000):
        t = ("A", "B", "C")[int(rng.integers(0, 3))]
        a, b = (int(x) for x in rng.choice(free, 2))
        if eid % 7 == 0 and edges:
            _, a, b, _ = edges[int(rng.integers(0, len(edges)))]  # a parallel edge: one entry, one vote
        edges.append((t, a, b, eid))
        g.create_edge(typ[t], a, b, eid)
    for k in rng.choice(len(edges), 300, replace=False):       # deleted edges
        t, a, b, eid = edges[k]
        g.delete_edge(typ[t], a, b, eid)
        edges[k] = None
    edges = [e for e in edges if e is not None]
    for v in doomed:
        g.delete_node(int(v))
    live = np.ones(n, dtype=bool)
    live[doomed] = False
    for labels, types, iters in [((), (), 10), ((), ("A",), 1), ((), ("B", "C"), 2), (("P",), (), 10), (("Q", "R"), ("A", "C"), 3),
                                 (("R",), ("B",), 10)]:
        sel = [e for e in edges if not types or e[0] in types]
        rp, ci = sym_csr(n, sel)
        active = None
        if labels:
            active = np.zeros(n, dtype=bool)
            for name in labels:
                active |= has[name]
            active &= live
        want, _, _ = cdlp_labels(n, rp, ci, iters, active)
        nodes, comm = g.algo_label_propagation(list(labels), list(types), iters)
        keep = live if active is None else active
        assert nodes.tolist() == np.flatnonzero(keep).tolist()
        if active is None:
            assert comm.tolist() == want[keep].tolist()
        else:
            rank = np.cumsum(active) - 1
            assert comm.tolist() == rank[want[keep]].tolist()
