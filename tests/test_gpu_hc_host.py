"""GPU: algo.HarmonicCentrality through the host layer (fh_algo_harmonic_centrality, algo_procedures.rs:2623-2784) — every
asserted relation of the reference's flow tests 03-08 (tests/golden/harmonic_flow.json, from its
tests/flow/test_harmonic_centrality.py), the unknown-relationship-type error, the empty graph, and a generated host graph with
deleted nodes and two labels against the numpy checker of tests/hc_check.py run with the equivalent mask."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hc_check import csr_of, harmonic, round_margin  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "harmonic_flow.json")))["cases"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """the k-th node of the case is node index k"""
    n = len(case["nodes"])
    g = host.Graph(hctx, max(n, 1))
    if n == 0:
        g.delete_node(0)
    at = {nd["name"]: k for k, nd in enumerate(case["nodes"])}
    labels, types = {}, {}
    for k, nd in enumerate(case["nodes"]):
        for l in nd["labels"]:
            if l not in labels:
                labels[l] = g.add_label(l)
            g.label_node(k, labels[l])
    for eid, (a, t, b) in enumerate(case["edges"]):
        if t not in types:
            types[t] = g.add_type(t)
        g.create_edge(types[t], at[a], at[b], eid)
    return g, at


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g, at = build(hctx, case)
    name = {k: n for n, k in at.items()}
    for q in case["queries"]:
        nodes, scores, reach = g.algo_harmonic_centrality(q["labels"], q["types"])
        assert nodes.tolist() == sorted(nodes.tolist())
        assert [name[v] for v in nodes.tolist()] == q["rows"]             # the row count, and who is in it
        sc = {name[v]: s for v, s in zip(nodes.tolist(), scores.tolist())}
        for a, b in q["greater"]:
            assert sc[a] > sc[b], (a, b, sc[a], sc[b])
        for z in q["zeros"]:
            assert sc[z] == 0.0, (z, sc[z])
        if "top" in q:
            assert max(sc, key=sc.get) == q["top"] and sorted(sc.values())[-1] > sorted(sc.values())[-2]
        if "differs_from" in q:
            d = q["differs_from"]
            n2, s2, _ = g.algo_harmonic_centrality(d["labels"], d["types"])
            full = {name[v]: s for v, s in zip(n2.tolist(), s2.tolist())}
            assert sc[d["node"]] != full[d["node"]]
        assert (reach >= 0).all() and len(reach) == len(nodes)


def test_unknown_relationship_type_is_an_error(hctx):
    g, _ = build(hctx, FLOW[0])
    with pytest.raises(host.HostError) as e:
        g.algo_harmonic_centrality([], ["NOPE"])
    assert "Relationship type 'NOPE' does not exist" in str(e.value)
    with pytest.raises(host.HostError):                                      # next to a known one, and before the empty-graph exit
        g.algo_harmonic_centrality([], ["EDGE", "NOPE"])
    empty, _ = build(hctx, {"nodes": [], "edges": []})
    with pytest.raises(host.HostError):
        empty.algo_harmonic_centrality([], ["NOPE"])
    # an unknown LABEL selects nothing; next to a known one it adds nothing
    assert len(g.algo_harmonic_centrality(["Nope"])[0]) == 0
    assert g.algo_harmonic_centrality(["Nope", "Node"])[0].tolist() == [0, 1, 2, 3]


def test_empty_graph_gives_no_rows(hctx):
    g, _ = build(hctx, {"nodes": [], "edges": []})
    nodes, scores, reach = g.algo_harmonic_centrality()
    assert len(nodes) == 0 and len(scores) == 0 and len(reach) == 0


def test_generated_host_graph_matches_the_checker(hctx):
    rng = np.random.default_rng(5)
    n = 1500
    g = host.Graph(hctx, n)
    lab = {name: g.add_label(name) for name in ("P", "Q")}
    typ = {name: g.add_type(name) for name in ("A", "B")}
    has = {name: rng.random(n) < p for name, p in (("P", 0.5), ("Q", 0.3))}
    for name, m in has.items():
        for v in np.flatnonzero(m):
            g.label_node(int(v), lab[name])
    doomed = rng.choice(n, 40, replace=False)                     # deleted later: they get no edges
    free = np.setdiff1d(np.arange(n), doomed)
    edges = []                                                      # (type, src, dst) — repeats are multi-edges: one entry
    for eid in range(4000):
        t = ("A", "B")[int(rng.integers(0, 2))]
        a, b = (int(x) for x in rng.choice(free, 2))
        if eid % 9 == 0 and edges:
            _, a, b = edges[int(rng.integers(0, len(edges)))]
        edges.append((t, a, b))
        g.create_edge(typ[t], a, b, eid)
    for v in doomed:
        g.delete_node(int(v))
    live = np.ones(n, dtype=bool)
    live[doomed] = False
    for labels, types in [((), ()), ((), ("A",)), (("P",), ()), (("P", "Q"), ("B",))]:
        sel = [e for e in edges if not types or e[0] in types]
        rp, ci = csr_of(n, [e[1] for e in sel], [e[2] for e in sel])
        active = None
        if labels:
            active = np.zeros(n, dtype=bool)
            for name in labels:
                active |= has[name]
            active &= live
        assert round_margin(n, rp, ci, active) > 1e-6
        ws, wr, _, _ = harmonic(n, rp, ci, active)
        nodes, scores, reach = g.algo_harmonic_centrality(list(labels), list(types))
        keep = live if active is None else active
        assert nodes.tolist() == np.flatnonzero(keep).tolist()
        err = float(np.abs(scores - ws[keep]).max())
        print(labels, types, "rows", len(nodes), "largest score difference", err)
        assert err <= 1e-9
        assert np.array_equal(reach, wr[keep])
