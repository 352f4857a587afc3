"""CPU: the checker of tests/pair_weights_check.py (what the GPU tests hold fgpu_pair_weights to) pinned to the reference's own
fixtures — followed by the Kruskal checker it reproduces the asserted results of tests/golden/msf_flow.json, followed by the
Dijkstra checker those of tests/golden/sppaths_flow.json — and to the pair rule tests/sppaths_enum_check.py already states."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_weights_check as pw  # noqa: E402
import sppaths_enum_check as enum  # noqa: E402
from msf_check import bits_of, key_of, msf  # noqa: E402
from sssp_check import sssp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSF_FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "msf_flow.json")))["cases"]
SP_FLOW = json.load(open(os.path.join(ROOT, "tests", "golden", "sppaths_flow.json")))["cases"]
U64 = np.uint64


def numeric(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def trees_of(n, rels, attr, maximize, active):
    """algo.MSF's answer from the checker's matrix: [node ids, kept relationship ids] per tree, by smallest node"""
    rows, cols, bits, kept, _ = pw.pair_weights(n, rels, attr, pw.OUT | pw.IN | (pw.NEGATE if maximize else 0), active, math.inf)
    kept_of = {(int(r), int(c)): int(k) for r, c, k in zip(rows, cols, kept)}
    fr, fc, _, comp = msf(n, rows, cols, bits, active)
    trees = {}
    for v in np.flatnonzero(active):
        trees.setdefault(int(comp[v]), ([], []))[0].append(int(v))
    for a, c in zip(fr.tolist(), fc.tolist()):
        assert kept_of[(a, c)] == kept_of[(c, a)]
        trees[int(comp[a])][1].append(kept_of[(a, c)])
    return [trees[k] for k in sorted(trees)]


@pytest.mark.parametrize("case", MSF_FLOW, ids=[c["name"] for c in MSF_FLOW])
def test_checker_then_kruskal_reproduces_the_msf_flow_cases(case):
    at = {name: k for k, name in enumerate(case["nodes"])}
    name = {k: nm for nm, k in at.items()}
    edges = case["edges"]
    n = len(case["nodes"])
    active = np.ones(n, dtype=bool)
    for q in case["queries"]:
        for nd in q.get("delete_nodes", []):
            active[at[nd]] = False
        attr = None
        if q["weight"] is not None:
            attr = {eid: float(e[3][q["weight"]]) for eid, e in enumerate(edges) if numeric(e[3].get(q["weight"]))}
        rels = [(t, at[a], at[b], eid) for eid, (a, t, b, _) in enumerate(edges) if not q["types"] or t in q["types"]]
        trees = trees_of(n, rels, attr, q["maximize"], active)
        if "trees" in q:
            assert [[[name[v] for v in nodes], eids] for nodes, eids in trees] == q["trees"]
            continue
        chosen = [e for _, eids in trees for e in eids]
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


DIRECTION = {"outgoing": pw.OUT, "incoming": pw.IN, "both": pw.OUT | pw.IN}


def sp_matrix(case):
    at = {name: k for k, (name, _) in enumerate(case["nodes"])}
    cfg = case["config"]
    prop = cfg["weight"]
    rels = [(t, at[a], at[b], eid) for eid, (a, t, b, _) in enumerate(case["edges"]) if not cfg["types"] or t in cfg["types"]]
    attr = None if not prop else {eid: float(e[3][prop]) for eid, e in enumerate(case["edges"]) if numeric(e[3].get(prop))}
    flags = DIRECTION[cfg["direction"]] | pw.DROP_NONFINITE | pw.REFUSE_NEGATIVE
    rows, cols, bits, kept, _ = pw.pair_weights(len(case["nodes"]), rels, attr, flags, None, 1.0)
    return at, len(case["nodes"]), rows, cols, bits, kept


@pytest.mark.parametrize("case", SP_FLOW, ids=[c["name"] for c in SP_FLOW])
def test_checker_then_dijkstra_reproduces_the_sppaths_flow_cases(case):
    at, n, rows, cols, bits, kept = sp_matrix(case)
    cfg, exp = case["config"], case["expect"]
    if "pairs" in exp:
        dist = {s: sssp(n, rows, cols, bits, s)[0] for s in range(n)}
        for s, t, want in exp["pairs"]:
            if want is None:
                assert np.isinf(dist[s][t]), (s, t)
            else:
                assert abs(dist[s][t] - want) <= exp["delta"], (s, t)
        return
    src, t = at[cfg["source"]], at[cfg["target"]]
    dist, parent, _ = sssp(n, rows, cols, bits, src)
    assert bool(np.isfinite(dist[t])) == exp["found"]
    if not exp["found"]:
        return
    path = [t]
    while path[-1] != src:
        path.append(int(parent[path[-1]]))
    path.reverse()
    if "nodes" in exp:
        assert [case["nodes"][v][0] for v in path] == exp["nodes"]
    if "hops" in exp:
        assert len(path) - 1 == exp["hops"]
    if "weight" in exp:
        assert abs(dist[t] - exp["weight"]) <= exp["delta"]
    kept_of = {(int(r), int(c)): int(k) for r, c, k in zip(rows, cols, kept)}
    if "cost" in exp and cfg["cost"]:
        cost = sum(case["edges"][kept_of[(a, b)]][3].get(cfg["cost"], 0) for a, b in zip(path, path[1:]))
        assert cost == exp["cost"]


@pytest.mark.parametrize("seed", enum.SEEDS)
def test_agrees_with_the_enumeration_checker_on_seeded_multigraphs(seed):
    n, edges, weights, _ = enum.seeded_graph(seed)
    for types in enum.REL_TYPES:
        order = enum.type_order(["R", "S"], list(types))
        rels = [(ty, s, d, i) for i, ty, s, d in edges if ty in order]
        for direction, reverse in (("outgoing", pw.IN), ("incoming", pw.OUT), ("both", pw.OUT | pw.IN)):
            want = enum.reverse_pair_weights(edges, order, direction, weights)
            rows, cols, bits, kept, stats = pw.pair_weights(n, rels, weights, reverse | pw.DROP_NONFINITE | pw.REFUSE_NEGATIVE)
            w = np.ones(len(rows)) if bits is None else bits.view(np.float64)
            got = {(int(r), int(c)): float(x) for r, c, x in zip(rows, cols, w)}
            assert got == want
            assert stats[3] == len(want) and stats[2] == stats[1] * (2 if direction == "both" else 1)
            by_id = {i: (s, d) for i, _, s, d in edges}
            for r, c, k in zip(rows.tolist(), cols.tolist(), kept.tolist()):
                assert set(by_id[k]) == {r, c}


def test_the_rules_one_by_one():
    inf, nan = math.inf, math.nan
    rels = [("A", 0, 1, 5), ("A", 0, 1, 9), ("B", 1, 0, 2), ("A", 2, 2, 3), ("A", 1, 3, 4), ("A", 0, 1, 5)]
    attr = {5: 2.0, 9: 2.0, 2: 3.0, 3: -1.0, 4: -0.0}
    rows, cols, bits, kept, st = pw.pair_weights(4, rels, attr, pw.OUT | pw.IN | pw.REFUSE_NEGATIVE)
    assert list(zip(rows.tolist(), cols.tolist(), kept.tolist())) == [(0, 1, 5), (1, 0, 5), (1, 3, 4), (3, 1, 4)]
    assert bits.tolist() == bits_of([2.0, 2.0, 0.0, 0.0]).tolist()          # the tie goes to the smaller id, -0.0 is +0.0
    assert st == [3, 4, 8, 4, 0, 0, 1, 3]                                     # the self-loop (negative) is neither counted nor refused
    with pytest.raises(pw.Refused) as e:                                      # NEGATE turns the positive values negative
        pw.pair_weights(4, rels, attr, pw.OUT | pw.NEGATE | pw.REFUSE_NEGATIVE)
    assert e.value.id == 2
    rows, cols, bits, kept, st = pw.pair_weights(4, rels, {9: nan, 2: -inf}, pw.IN, None, inf)
    assert list(zip(rows.tolist(), cols.tolist(), kept.tolist())) == [(0, 1, 2), (1, 0, 5), (3, 1, 4)]
    assert key_of(bits_of([inf]))[0] < key_of(bits_of([nan]))[0] and st[5] == 2 and st[4] == 0
    _, _, _, _, st = pw.pair_weights(4, rels, {9: nan, 2: -inf}, pw.IN | pw.DROP_NONFINITE, None, inf)
    assert st[4] == 4 and st[2] == 0 and st[3] == 0
    rows, cols, bits, kept, st = pw.pair_weights(4, rels, None, pw.OUT, np.array([True, True, True, False]))
    assert bits is None and list(zip(rows.tolist(), cols.tolist(), kept.tolist())) == [(0, 1, 5), (1, 0, 2)] and st[1] == 3
