"""GPU: algo.maxFlow through the host layer (fh_algo_maxflow, algo_procedures.rs:2786-3248) — what the reference's flow tests
assert (tests/golden/maxflow_flow.json, from its tests/flow/test_maxflow.py: tests 01b, 01c, 02 to 07, 12 to 37), then the paths
those graphs do not reach: node ids compacted because of a deleted node, pending additions and deletions, the order of the
returned relationships, and the remaining failures.  Every returned flow is certified by tests/maxflow_check.py."""
import json
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maxflow_check import certify, dinic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "maxflow_flow.json")))["cases"]
BIG = float(2**31 - 1)


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, case):
    """node k of the case is node id k, edge k relationship id k; the case's deletions applied"""
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
    for eid in case.get("delete_edges", []):
        a, t, b, _ = case["edges"][eid]
        g.delete_edge(types[t], at[a], at[b], eid)
    for name in case.get("delete_nodes", []):
        g.delete_node(at[name])
    return g, at


def call(g, at, case):
    cfg = case["config"]
    caps = None
    known = case.get("attribute_known", False)
    if cfg["capacity"] is not None:
        caps = {eid: e[3][cfg["capacity"]] for eid, e in enumerate(case["edges"]) if cfg["capacity"] in e[3]}
        known = known or bool(caps)
    return g.algo_maxflow([at[s] for s in cfg["sources"]], [at[t] for t in cfg["targets"]], cfg["types"], caps,
                          cfg.get("default"), cfg["labels"], attribute_exists=known)


def network_of(case, at):
    """(n, rows, cols, caps, src, sink, edge ids) of the network the procedure solves for a case WITHOUT an error: the selected
    type's surviving edges between selected nodes, capacities resolved, super nodes appended behind the node ids"""
    cfg = case["config"]
    label_of = dict((name, label) for name, label in case["nodes"])
    gone = set(case.get("delete_edges", []))
    rows, cols, caps, ids = [], [], [], []
    for eid, (a, t, b, attrs) in enumerate(case["edges"]):
        if eid in gone or t != cfg["types"][0]:
            continue
        if cfg["labels"] and (label_of[a] not in cfg["labels"] or label_of[b] not in cfg["labels"]):
            continue
        c = attrs.get(cfg["capacity"])
        if not (isinstance(c, (int, float)) and not isinstance(c, bool) and c >= 0):
            c = cfg["default"]
        rows.append(at[a]); cols.append(at[b]); caps.append(float(c)); ids.append(eid)
    n = len(case["nodes"])
    src, sink = at[cfg["sources"][0]], at[cfg["targets"][0]]
    if len(cfg["sources"]) > 1:
        src, n = n, n + 1
        for s in cfg["sources"]:
            rows.append(src); cols.append(at[s]); caps.append(BIG); ids.append(None)
    if len(cfg["targets"]) > 1:
        sink, n = n, n + 1
        for t in cfg["targets"]:
            rows.append(at[t]); cols.append(sink); caps.append(BIG); ids.append(None)
    return n, rows, cols, caps, src, sink, ids


def certify_result(case, at, nodes, edges, flows, value, exact=True, tol=0.0):
    """the returned relationships with their flows, completed by the super arcs' flows (what enters a source from the super
    source is what the source hands on), are a maximum flow of the case's network"""
    n, rows, cols, caps, src, sink, ids = network_of(case, at)
    cfg = case["config"]
    pos = {eid: k for k, eid in enumerate(ids) if eid is not None}
    assert all(int(e) in pos for e in edges)                                   # no super arc, no other type, nothing deleted
    f = {(rows[pos[int(e)]], cols[pos[int(e)]]): float(x) for e, x in zip(edges, flows)}
    assert len(f) == len(edges) and all(x != 0 for x in flows)
    ends = sorted({v for uv in f for v in uv})
    assert nodes.tolist() == ends                                              # ascending endpoints of the flow's relationships
    assert [int(e) for e in edges] == sorted((int(e) for e in edges), key=lambda e: (rows[pos[e]], cols[pos[e]]))
    net = {}
    for (u, v), x in f.items():
        net[u] = net.get(u, 0.0) + x
        net[v] = net.get(v, 0.0) - x
    if len(cfg["sources"]) > 1:
        for s in cfg["sources"]:
            if net.get(at[s], 0.0) > 0:
                f[(src, at[s])] = net[at[s]]
    if len(cfg["targets"]) > 1:
        for t in cfg["targets"]:
            if net.get(at[t], 0.0) < 0:
                f[(at[t], sink)] = -net[at[t]]
    order = sorted(f)
    certify(n, rows, cols, caps, src, sink, value, [u for u, _ in order], [v for _, v in order], [f[uv] for uv in order],
            exact=exact, tol=tol)
    return dinic(n, rows, cols, caps, src, sink)


@pytest.mark.parametrize("case", FLOW, ids=[c["name"] for c in FLOW])
def test_reference_flow_cases(hctx, case):
    g, at = build(hctx, case)
    exp = case["expect"]
    if "error" in exp:
        with pytest.raises(host.HostError, match=exp["error"]):
            call(g, at, case)
        return
    nodes, edges, flows, value = call(g, at, case)
    print(f"{case['name']}: maxFlow={value!r} edges={edges.tolist()} flows={flows.tolist()} nodes={nodes.tolist()}")
    if "maxFlow" in exp:
        if "places" in exp:
            assert round(abs(value - exp["maxFlow"]), exp["places"]) == 0      # assertAlmostEqual(.., places)
        else:
            assert value == exp["maxFlow"]
    if "edgeFlows" in exp:
        assert flows.tolist() == exp["edgeFlows"]
    if "nodes" in exp:
        assert nodes.tolist() == exp["nodes"] and edges.tolist() == exp["edges"]
    if "node_count" in exp:
        assert len(nodes) == exp["node_count"]
    if "max_node_id" in exp:
        assert len(nodes) > 0 and int(nodes.max()) <= exp["max_node_id"]
        for e in edges.tolist():
            a, _, b, _ = case["edges"][e]
            assert at[a] <= exp["max_node_id"] and at[b] <= exp["max_node_id"]
    exact = "places" not in exp
    tol = 0.0 if exact else 5e-6 * max([float(e[3]["cap"]) for e in case["edges"] if isinstance(e[3].get("cap"), (int, float))] +
                                       [float(case["config"].get("default", 0))])
    assert abs(certify_result(case, at, nodes, edges, flows, value, exact=exact, tol=tol) - value) <= tol


def random_case(rng, n, m, extra_nodes=0):
    key = np.unique(rng.integers(0, n * n, m))
    rows, cols = key // n, key % n
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    order = rng.permutation(len(rows))                                         # relationship ids in no particular order
    nodes = [[f"v{k}", "Node"] for k in range(n + extra_nodes)]
    edges = [[f"v{rows[k]}", "PIPE", f"v{cols[k]}", {"cap": int(rng.integers(0, 40))}] for k in order]
    return nodes, edges


def test_deleted_node_compacts_the_ids(hctx):
    """a deleted node switches the procedure to compact ids (the sorted distinct ends, sources and targets): the result is the
    same maximum flow, reported in node ids"""
    rng = np.random.default_rng(51)
    nodes, edges = random_case(rng, 60, 400, extra_nodes=3)
    for multi in (False, True):
        case = {"nodes": nodes, "edges": edges, "delete_nodes": ["v60", "v62"],
                "config": {"sources": ["v3", "v9"] if multi else ["v3"], "targets": ["v50", "v7", "v44"] if multi else ["v50"],
                           "types": ["PIPE"], "capacity": "cap", "labels": []}}
        g, at = build(hctx, case)
        nodes_out, eids, flows, value = call(g, at, case)
        assert certify_result(case, at, nodes_out, eids, flows, value) == value and value > 0
        keep = dict(case, delete_nodes=[])                                     # the identity path on the same graph
        g2, _ = build(hctx, keep)
        assert call(g2, at, keep)[3] == value


def test_pending_additions_and_deletions_are_applied(hctx):
    rng = np.random.default_rng(52)
    nodes, edges = random_case(rng, 40, 300)
    case = {"nodes": nodes, "edges": edges, "config": {"sources": ["v0"], "targets": ["v39"], "types": ["PIPE"],
                                                       "capacity": "cap", "labels": []}}
    g, at = build(hctx, case)
    g.commit()
    # after the commit: a tenth of the relationships deleted, a few new ones added, nothing flushed
    gone = list(range(0, len(edges), 10))
    for eid in gone:
        a, t, b, _ = edges[eid]
        g.delete_edge(0, at[a], at[b], eid)
    have = {(e[0], e[2]) for e in edges}
    fresh = [[f"v{a}", "PIPE", f"v{b}", {"cap": 25}] for a, b in ((0, 17), (17, 39), (5, 39), (0, 5)) if (f"v{a}", f"v{b}") not in have]
    for k, (a, t, b, _) in enumerate(fresh):
        g.create_edge(0, at[a], at[b], len(edges) + k)
    now = dict(case, edges=edges + fresh, delete_edges=gone)
    nodes_out, eids, flows, value = call(g, at, now)
    assert certify_result(now, at, nodes_out, eids, flows, value) == value and value > 0
    assert not set(eids.tolist()) & set(gone)


def test_a_node_listed_twice_hangs_under_the_super_node_once(hctx):
    case = {"nodes": [["A", "Node"], ["B", "Node"], ["C", "Node"], ["D", "Node"]],
            "edges": [["A", "PIPE", "C", {"cap": 5}], ["B", "PIPE", "C", {"cap": 3}], ["C", "PIPE", "D", {"cap": 20}]]}
    g, at = build(hctx, case)
    caps = {0: 5, 1: 3, 2: 20}
    for sources, targets, want in (([0, 1, 0], [3], 8.0), ([0, 0], [3], 5.0), ([0, 1], [3, 3], 8.0), ([1, 1, 1], [2, 3, 2], 3.0)):
        nodes, eids, flows, value = g.algo_maxflow(sources, targets, ["PIPE"], caps)
        assert value == want
        assert int(nodes.max()) <= 3 and set(eids.tolist()) <= {0, 1, 2}       # no super node, no super arc
        if targets[0] == 3:
            assert float(flows[eids.tolist().index(2)]) == want                # everything arrives over C -> D


def test_remaining_failures(hctx):
    case = {"nodes": [["A", "Node"], ["B", "Node"]], "edges": [["A", "PIPE", "B", {"cap": 2}]]}
    g, at = build(hctx, case)
    caps = {0: 2}
    with pytest.raises(host.HostError, match="exactly one relationship type"):
        g.algo_maxflow([0], [1], [], caps)
    with pytest.raises(host.HostError, match="exactly one relationship type"):
        g.algo_maxflow([0], [1], ["PIPE", "PIPE"], caps)
    with pytest.raises(host.HostError, match="unknown"):
        g.algo_maxflow([0], [1], ["FAKE"], caps)
    with pytest.raises(host.HostError, match="defaultCapacity"):
        g.algo_maxflow([0], [1], ["PIPE"], caps, default_capacity=-1)
    with pytest.raises(host.HostError, match="invalid or missing attribute"):
        g.algo_maxflow([0], [1], ["PIPE"], None)                               # the graph does not know the attribute, no default
    with pytest.raises(host.HostError, match="invalid or missing attribute"):
        g.algo_maxflow([0], [1], ["PIPE"], {0: -2})                            # a negative capacity is no capacity
    nodes, eids, flows, value = g.algo_maxflow([0], [1], ["PIPE"], {0: -2}, default_capacity=1.5)
    assert value == 1.5 and flows.tolist() == [1.5] and eids.tolist() == [0] and nodes.tolist() == [0, 1]
    nodes, eids, flows, value = g.algo_maxflow([0], [1], ["PIPE"], None, default_capacity=3)   # unknown attribute, default given
    assert value == 3 and flows.tolist() == [3]
