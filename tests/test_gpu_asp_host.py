"""GPU: AllShortestPathsOp through the host layer (fh_all_shortest_paths; all_shortest_paths.rs:82-303) — what the reference's flow
tests assert (tests/golden/asp_flow.json, from its tests/flow/test_all_shortest_paths.py: tests 02, 05, 06 and 07), compared
as sorted relationship-id sets, then the exact emission sequence and per-path edge order against the restatement of the
operator in tests/asp_check.py (reference_paths) on those graphs and on seeded random multigraphs."""
import json
import os
import random
import sys

import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asp_check import random_multigraph, reference_paths  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asp_flow.json")))


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, n, edges):
    """edges [(id, type, src, dst)]: the types are created in the order they first appear, one bulk insert per type"""
    g = host.Graph(hctx, max(n, 1))
    order = list(dict.fromkeys(t for _, t, _, _ in edges))
    for t in order:
        tid = g.add_type(t)
        mine = [e for e in edges if e[1] == t]
        g.create_edges(tid, [s for _, _, s, _ in mine], [d for _, _, _, d in mine], [i for i, _, _, _ in mine])
    return g


def golden_graph(hctx, name):
    g = GOLD["graphs"][name]
    edges = [(i, t, s, d) for i, (s, t, d) in enumerate(g["edges"])]
    return build(hctx, len(g["nodes"]), edges), len(g["nodes"]), edges


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_reference_flow_cases(hctx, case):
    g, n, edges = golden_graph(hctx, case["graph"])
    length, paths = g.all_shortest_paths(case["src"], case["dst"], case["types"], case["bidirectional"], case["reversed"],
                                         case["max_hops"])
    assert sorted(sorted(p) for p in paths) == case["expect_id_sets"]
    assert length == (len(case["expect_id_sets"][0]) if case["expect_id_sets"] else -1)
    assert paths == reference_paths(n, edges, case["src"], case["dst"], case["types"], case["bidirectional"], case["reversed"],
                                    case["max_hops"])


def hold(g, n, edges, src, dst, types, bidirectional, reversed, max_hops):
    want = reference_paths(n, edges, src, dst, list(types), bidirectional, reversed, max_hops)
    length, got = g.all_shortest_paths(src, dst, types, bidirectional, reversed, max_hops)
    assert got == want, (src, dst, types, bidirectional, reversed, max_hops)
    assert length == (len(want[0]) if want else -1)
    return want


@pytest.mark.parametrize("graph", ["acyclic", "cyclic", "acyclic_07"])
def test_exact_sequence_on_the_golden_graphs(hctx, graph):
    g, n, edges = golden_graph(hctx, graph)
    found = 0
    for bidirectional, reversed in ((False, False), (False, True), (True, False)):
        for types in ((), ("E2", "E"), ("E",)):
            for s in range(n):
                for d in range(n):
                    found += len(hold(g, n, edges, s, d, types, bidirectional, reversed, None))
    assert found > 50


def test_exact_sequence_on_random_multigraphs(hctx):
    found = cycles = cut = 0
    for seed in range(50):
        rng = random.Random(0x51DE + seed)
        n = rng.randint(3, 40)
        edges = random_multigraph(rng, n, rng.randint(n, 4 * n), ["A", "B", "C"])
        g = build(hctx, n, edges)
        bidirectional = seed % 3 == 1
        reversed = seed % 3 == 2
        types = [(), ("C", "A"), ("B",), ("A", "nope", "B", "C")][seed % 4]
        for k in range(8):
            s = rng.randrange(n)
            d = s if k < 2 else rng.randrange(n)
            want = hold(g, n, edges, s, d, types, bidirectional, reversed, None)
            found += len(want)
            cycles += len(want) if s == d else 0
            if want:   # the max_hops cut: L keeps every path, L - 1 leaves none
                L = len(want[0])
                assert hold(g, n, edges, s, d, types, bidirectional, reversed, L) == want
                assert hold(g, n, edges, s, d, types, bidirectional, reversed, L - 1) == []
                cut += 1
    assert found > 300 and cycles > 20 and cut > 100


def test_limit_truncates_the_same_sequence(hctx):
    # a chain of four diamonds whose arms are double edges: 4^4 paths
    edges, eid = [], 0
    for k in range(4):
        a, top, bottom, b = 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3
        for s, d in ((a, top), (a, top), (a, bottom), (a, bottom), (top, b), (bottom, b)):
            edges.append((eid, "R" if eid % 3 else "S", s, d))
            eid += 1
    n = 13
    g = build(hctx, n, edges)
    want = reference_paths(n, edges, 0, 12, [], False, False, None)
    assert len(want) == 4 ** 4
    for limit in (1, 7, 255, 256, 1000):
        length, got = g.all_shortest_paths(0, 12, limit=limit)
        assert length == 8 and got == want[:limit]
    assert g.all_shortest_paths(0, 12, limit=0)[1] == want


def test_out_of_range_and_unknown_types_give_no_row(hctx):
    g, n, edges = golden_graph(hctx, "acyclic")
    assert g.all_shortest_paths(0, 99) == (-1, [])
    assert g.all_shortest_paths(99, 0) == (-1, [])
    assert g.all_shortest_paths(0, 3, types=("nope",)) == (-1, [])
    assert g.all_shortest_paths(0, 3, max_hops=0) == (-1, [])
