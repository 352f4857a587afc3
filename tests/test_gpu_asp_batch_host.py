"""GPU: AllShortestPathsOp over a parent batch of rows through the host layer (fh_all_shortest_paths_batch): every row equals
the one-row call and the restatement of the operator in tests/asp_check.py (reference_paths) — the same paths, in the same
sequence and per-path edge order — on the golden graphs and on seeded random multigraphs, all rows of a graph in one batch."""
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


def hold(g, n, edges, queries, types, bidirectional, reversed, max_hops, single=True):
    """one batch of `queries` against reference_paths per row and (single=True) against the one-row call; returns the rows' paths"""
    got = g.all_shortest_paths_batch([s for s, _ in queries], [d for _, d in queries], types, bidirectional, reversed, max_hops)
    assert len(got) == len(queries)
    for (s, d), (length, paths) in zip(queries, got):
        want = reference_paths(n, edges, s, d, list(types), bidirectional, reversed, max_hops)
        assert paths == want, (s, d, types, bidirectional, reversed, max_hops)
        assert length == (len(want[0]) if want else -1)
        if single:
            assert (length, paths) == g.all_shortest_paths(s, d, types, bidirectional, reversed, max_hops)
    return [paths for _, paths in got]


@pytest.mark.parametrize("graph", ["acyclic", "cyclic", "acyclic_07"])
def test_every_ordered_pair_of_the_golden_graphs_in_one_batch(hctx, graph):
    g, n, edges = golden_graph(hctx, graph)
    queries = [(s, d) for s in range(n) for d in range(n)]
    found = 0
    for bidirectional, reversed in ((False, False), (False, True), (True, False)):
        for types in ((), ("E2", "E"), ("E",)):
            found += sum(len(p) for p in hold(g, n, edges, queries, types, bidirectional, reversed, None))
    assert found > 50


def test_random_multigraphs_all_queries_of_a_seed_in_one_batch(hctx):
    found = cycles = cut = 0
    for seed in range(50):
        rng = random.Random(0x51DE + seed)
        n = rng.randint(3, 40)
        edges = random_multigraph(rng, n, rng.randint(n, 4 * n), ["A", "B", "C"])
        g = build(hctx, n, edges)
        bidirectional = seed % 3 == 1
        reversed = seed % 3 == 2
        types = [(), ("C", "A"), ("B",), ("A", "nope", "B", "C")][seed % 4]
        queries = []
        for k in range(8):
            s = rng.randrange(n)
            queries.append((s, s if k < 2 else rng.randrange(n)))
        rows = hold(g, n, edges, queries, types, bidirectional, reversed, None)
        found += sum(len(p) for p in rows)
        cycles += sum(len(p) for (s, d), p in zip(queries, rows) if s == d)
        for L in sorted({len(p[0]) for p in rows if p}):   # the max_hops cut: L keeps the rows of length <= L, L - 1 drops those of L
            at = hold(g, n, edges, queries, types, bidirectional, reversed, L, single=False)
            below = hold(g, n, edges, queries, types, bidirectional, reversed, L - 1, single=False)
            for p, a, b in zip(rows, at, below):
                if p and len(p[0]) == L:
                    assert a == p and b == []
                    cut += 1
    assert found > 300 and cycles > 20 and cut > 100


def test_limit_is_applied_per_row(hctx):
    # a chain of four diamonds whose arms are double edges: 4^4 paths; node 13 is out of reach
    edges, eid = [], 0
    for k in range(4):
        a, top, bottom, b = 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3
        for s, d in ((a, top), (a, top), (a, bottom), (a, bottom), (top, b), (bottom, b)):
            edges.append((eid, "R" if eid % 3 else "S", s, d))
            eid += 1
    n = 14
    g = build(hctx, n, edges)
    want = reference_paths(n, edges, 0, 12, [], False, False, None)
    assert len(want) == 4 ** 4
    for limit in (1, 7, 256, 0):
        got = g.all_shortest_paths_batch([0, 0, 0, 0], [12, 12, 13, 12], limit=limit)
        keep = want[:limit] if limit else want
        assert got == [(8, keep), (8, keep), (-1, []), (8, keep)]


def test_rows_that_never_reach_the_device_do_not_disturb_their_neighbours(hctx):
    g, n, edges = golden_graph(hctx, "acyclic")
    want = g.all_shortest_paths(0, 3)
    assert want[0] > 0
    got, st = g.all_shortest_paths_batch([0, 0, 99, 0, 2**40], [3, 99, 0, 3, 0], stats=True)
    assert got == [want, (-1, []), (-1, []), want, (-1, [])] and st["device_calls"] == 1
    got, st = g.all_shortest_paths_batch([0, 0], [3, 3], types=("nope",), stats=True)
    assert got == [(-1, []), (-1, [])] and st["device_calls"] == 0
    got, st = g.all_shortest_paths_batch([99], [0], stats=True)
    assert got == [(-1, [])] and st["device_calls"] == 0
    assert g.all_shortest_paths_batch([], []) == []
    assert g.all_shortest_paths_batch([0, 0], [3, 3], max_hops=0) == [(-1, []), (-1, [])]
    # a deleted node: its rows are empty, as the one-row call's, the others unchanged
    g2, n2, edges2 = golden_graph(hctx, "cyclic")
    queries = [(s, d) for s in range(n2) for d in range(n2)]
    before = g2.all_shortest_paths_batch([s for s, _ in queries], [d for _, d in queries])
    gone = n2 - 1
    incident = [(t, s, d, i) for i, t, s, d in edges2 if gone in (s, d)]
    tids = {t: k for k, t in enumerate(dict.fromkeys(t for _, t, _, _ in edges2))}
    for t, s, d, i in incident:
        g2.delete_edge(tids[t], s, d, i)
    g2.delete_node(gone)
    after = g2.all_shortest_paths_batch([s for s, _ in queries], [d for _, d in queries])
    for (s, d), row in zip(queries, after):
        assert row == g2.all_shortest_paths(s, d)
        if gone in (s, d):
            assert row == (-1, [])
    assert any(a != b for a, b in zip(before, after)) and any(a == b and a[0] > 0 for a, b in zip(before, after))


def test_one_device_call_serves_every_ordered_pair(hctx):
    rng = random.Random(0xA11)
    n = 40
    edges = random_multigraph(rng, n, 3 * n, ["A", "B"])
    g = build(hctx, n, edges)
    queries = [(s, d) for s in range(n) for d in range(n)]
    got, st = g.all_shortest_paths_batch([s for s, _ in queries], [d for _, d in queries], stats=True)
    assert st["device_calls"] == 1
    found = 0
    for (s, d), (length, paths) in zip(queries, got):
        want = reference_paths(n, edges, s, d, [], False, False, None)
        assert paths == want and length == (len(want[0]) if want else -1), (s, d)
        found += len(paths)
    assert found > 1000
