"""GPU: algo.WCC through the host layer (fh_algo_wcc, algo_procedures.rs:789-880) — the reference's flow cases
(tests/golden/wcc_flow.json, from its tests/flow/test_wcc.py), the compact componentIds of a label-filtered run, deleted
nodes, and a random host graph against the numpy checker of tests/wcc_check.py."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wcc_check import csr_of, wcc_labels  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "wcc_flow.json")))["cases"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node with property id = k is node index k - 1"""
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


def grouped(nodes, comp, id_of=lambda v: int(v) + 1):
    """get_components of the flow test: the ids of every component, sorted by (size, ids)"""
    by = {}
    for v, c in zip(nodes.tolist(), comp.tolist()):
        by.setdefault(c, []).append(id_of(v))
    return sorted((sorted(x) for x in by.values()), key=lambda x: (len(x), x))


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g = build(hctx, case)
    for q in case["queries"]:
        nodes, comp = g.algo_wcc(q["labels"], q["types"])
        assert nodes.tolist() == sorted(nodes.tolist())
        assert grouped(nodes, comp) == q["components"], q


def test_component_ids_unlabelled_are_node_ids_labelled_are_compact(hctx):
    case = next(c for c in FLOW if c["name"] == "labels_x_types")
    g = build(hctx, case)
    nodes, comp = g.algo_wcc([], ["R2"])
    # unlabelled: the representative's node id (the smallest index of the component)
    assert dict(zip(nodes.tolist(), comp.tolist())) == {0: 0, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 4, 8: 4}
    # L1 + L2 over R1 selects ids {1..6, 9} = indices {0..5, 8}; their compact ranks are 0..6, and the componentId is the
    # representative's rank: [1,2,3,9] -> rank of index 0, [4,5] -> rank of index 3, [6] -> rank of index 5
    nodes, comp = g.algo_wcc(["L1", "L2"], ["R1"])
    assert nodes.tolist() == [0, 1, 2, 3, 4, 5, 8]
    assert comp.tolist() == [0, 0, 0, 3, 3, 5, 0]
    # L2 alone: indices {3, 4, 5, 8} -> ranks 0..3; [4,5] -> 0, [6] -> 2, [9] -> 3
    nodes, comp = g.algo_wcc(["L2"], ["R1"])
    assert nodes.tolist() == [3, 4, 5, 8] and comp.tolist() == [0, 0, 2, 3]
    # unknown labels select nothing; an unknown label next to a known one adds nothing; unknown types add no edges
    assert len(g.algo_wcc(["Nope"], [])[0]) == 0
    assert g.algo_wcc(["Nope", "L2"], ["R1"])[1].tolist() == [0, 0, 2, 3]
    nodes, comp = g.algo_wcc([], ["Nope"])
    assert nodes.tolist() == list(range(9)) and comp.tolist() == list(range(9))


def test_deleted_nodes_leave_the_output(hctx):
    case = next(c for c in FLOW if c["name"] == "unlabeled")
    g = build(hctx, case)
    g.delete_node(5)                                           # the isolated node 6
    nodes, comp = g.algo_wcc()
    assert nodes.tolist() == [0, 1, 2, 3, 4]
    assert comp.tolist() == [0, 0, 0, 3, 3]
    for v in (0, 1, 2, 4):                                    # (marked deleted; their edges stay in the matrix, as in the reference)
        g.delete_node(v)
    nodes, comp = g.algo_wcc()
    assert nodes.tolist() == [3] and comp.tolist() == [3]
    g.delete_node(3)
    assert len(g.algo_wcc()[0]) == 0                           # no live node: an empty result


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
    for eid in range(4000):
        t = ("A", "B", "C")[int(rng.integers(0, 3))]
        a, b = (int(x) for x in rng.choice(free, 2))
        if eid % 7 == 0 and edges:
            _, a, b, _ = edges[int(rng.integers(0, len(edges)))]  # a parallel edge
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
    for labels, types in [((), ()), ((), ("A",)), ((), ("B", "C")), (("P",), ()), (("Q", "R"), ("A", "C")), (("R",), ("B",))]:
        sel = [e for e in edges if not types or e[0] in types]
        rp, ci = csr_of(n, [e[1] for e in sel], [e[2] for e in sel])
        active = None
        if labels:
            active = np.zeros(n, dtype=bool)
            for name in labels:
                active |= has[name]
            active &= live
        want = wcc_labels(n, rp, ci, active)
        nodes, comp = g.algo_wcc(list(labels), list(types))
        keep = live if active is None else active
        assert nodes.tolist() == np.flatnonzero(keep).tolist()
        if active is None:
            assert comp.tolist() == want[keep].tolist()
        else:
            rank = np.cumsum(active) - 1
            assert comp.tolist() == rank[want[keep]].tolist()
