"""GPU: algo.MSF through the host layer (fh_algo_msf, algo_procedures.rs:1272-1857) — what the reference's flow tests assert on
their deterministic cases (tests/golden/msf_flow.json, from its tests/flow/test_msf.py), and a generated multigraph with two
types, parallel edges, missing weights and pending deletions / additions against a plain-Python restatement of the pair rule
plus the Kruskal checker of tests/msf_check.py."""
import json
import math
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of, msf  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "msf_flow.json")))["cases"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node k of the case is node id k, edge k relationship id k"""
    n = len(case["nodes"])
    g = host.Graph(hctx, max(n, 1))
    if n == 0:
        g.delete_node(0)
    at = {name: k for k, name in enumerate(case["nodes"])}
    types = {}
    for eid, (a, t, b, _) in enumerate(case["edges"]):
        if t not in types:
            types[t] = g.add_type(t)
        g.create_edge(types[t], at[a], at[b], eid)
    return g, at


def numeric(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g, at = build(hctx, case)
    name = {k: n for n, k in at.items()}
    edges = case["edges"]
    for q in case["queries"]:
        for nd in q.get("delete_nodes", []):
            g.delete_node(at[nd])
        weights = None
        if q["weight"] is not None:
            weights = {eid: e[3][q["weight"]] for eid, e in enumerate(edges) if numeric(e[3].get(q["weight"]))}
        trees = g.algo_msf((), q["types"], q["maximize"], weights)
        for nodes, eids in trees:
            assert len(eids) == len(nodes) - 1 and nodes.tolist() == sorted(nodes.tolist())
        assert [int(t[0][0]) for t in trees] == sorted(int(t[0][0]) for t in trees)
        if "trees" in q:
            assert [[[name[v] for v in nodes.tolist()], eids.tolist()] for nodes, eids in trees] == q["trees"]
            continue
        chosen = [int(e) for _, eids in trees for e in eids.tolist()]
        rows = [[edges[e][1] if col == "type" else edges[e][3].get(col) for col in q["return"]] for e in chosen]
        if "order_by" in q:
            k = q["return"].index(q["order_by"])
            rows.sort(key=lambda r: (r[k] is None, r[k] if r[k] is not None else 0))
        if "rows" in q:
            assert rows == q["rows"]
        if "count" in q:
            assert len(rows) == q["count"]
        for r in q.get("contains", []):
            assert r in rows
        if "count_among" in q:
            assert sum(1 for r in rows if r[0] in q["count_among"]["values"]) == q["count_among"]["n"]


def test_unknown_type_and_empty_graph(hctx):
    g, _ = build(hctx, FLOW[0])
    with pytest.raises(host.HostError) as e:
        g.algo_msf((), ["FAKE"])
    assert "Relationship type 'FAKE' does not exist" in str(e.value)
    with pytest.raises(host.HostError):
        g.algo_msf((), ["R", "FAKE"])
    empty, _ = build(hctx, {"nodes": [], "edges": []})
    assert empty.algo_msf() == []
    with pytest.raises(host.HostError):                       # the type check comes before the empty-graph exit
        empty.algo_msf((), ["FAKE"])
    assert g.algo_msf(["Nope"]) == []                         # an unknown label selects no node


def expected_trees(n, edges, selected, types, maximize, weights):
    """the pair rule in plain Python, then the checker.  edges: (type, src, dst, id) effective relationships"""
    best = {}
    for t, a, b, eid in edges:
        if (types and t not in types) or a == b or not (selected[a] and selected[b]):
            continue
        if weights is None:
            s = 1.0
        elif eid not in weights:
            s = math.inf
        else:
            s = -float(weights[eid]) if maximize else float(weights[eid])
        key = (min(a, b), max(a, b))
        if key not in best or s < best[key][0] or (s == best[key][0] and eid < best[key][1]):
            best[key] = (s, eid)
    lo = np.array([k[0] for k in best], dtype=np.int64)
    hi = np.array([k[1] for k in best], dtype=np.int64)
    b = bits_of(np.array([best[k][0] for k in best], dtype=np.float64))
    fr, fc, _, comp = msf(n, np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([b, b]), selected)
    trees = {}
    for v in np.flatnonzero(selected):
        trees.setdefault(int(comp[v]), ([], []))[0].append(int(v))
    for a, c in zip(fr.tolist(), fc.tolist()):
        trees[int(comp[a])][1].append(best[(a, c)][1])
    return [trees[k] for k in sorted(trees)]


def test_generated_multigraph_with_pending_changes(hctx):
    rng = np.random.default_rng(23)
    n = 300
    g = host.Graph(hctx, n)
    lab = {name: g.add_label(name) for name in ("P", "Q")}
    typ = {name: g.add_type(name) for name in ("A", "B")}
    has = {name: rng.random(n) < p for name, p in (("P", 0.5), ("Q", 0.3))}
    for name, m in has.items():
        for v in np.flatnonzero(m):
            g.label_node(int(v), lab[name])
    edges, weights = [], {}

    def add(eid):
        t = ("A", "B")[int(rng.integers(0, 2))]
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if eid % 4 == 0 and edges:                              # a parallel edge, either direction, either type
            _, a, b, _ = edges[int(rng.integers(0, len(edges)))]
            if eid % 8 == 0:
                a, b = b, a
        edges.append((t, a, b, eid))
        g.create_edge(typ[t], a, b, eid)
        if eid % 3:                                             # a third of the relationships have no weight
            weights[eid] = [0.0, -0.0, 1.0, 2.5, -4.0, 7, 7.0, 1e300][int(rng.integers(0, 8))]

    for eid in range(700):
        add(eid)
    g.commit()
    doomed = [edges[i] for i in rng.choice(len(edges), 120, replace=False)]   # pending deletions ...
    for t, a, b, eid in doomed:
        g.delete_edge(typ[t], a, b, eid)
    gone = {e[3] for e in doomed}
    edges[:] = [e for e in edges if e[3] not in gone]
    for eid in range(700, 850):                                               # ... and pending additions
        add(eid)
    live = np.ones(n, dtype=bool)
    runs = 0
    for labels in [(), ("P",), ("P", "Q")]:
        selected = live.copy()
        if labels:
            selected = np.zeros(n, dtype=bool)
            for name in labels:
                selected |= has[name]
        for types in [(), ("A",), ("B",)]:
            for maximize in (False, True):
                for w in (weights, None):
                    if w is None and maximize:
                        continue
                    want = expected_trees(n, edges, selected, types, maximize, w)
                    got = g.algo_msf(list(labels), list(types), maximize, w)
                    assert [(a.tolist(), b.tolist()) for a, b in got] == [(a, b) for a, b in want]
                    runs += 1
    assert runs == 27
