"""GPU: shortestPath() through the host layer (fh_shortest_path, fh_shortest_path_batch): the golden cases of the reference's flow
tests, and eval_batch == eval_row == the restatement in tests/spath_check.py (reference_path), row by row, on a seeded
multi-type graph with multi-edge pairs, uncommitted deltas, deleted nodes, out-of-range ids and Null endpoints."""
import json
import os
import random
import sys

import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asp_check import random_multigraph  # noqa: E402
from spath_check import reference_path  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shortest_path_flow.json")))


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, n, edges):
    """edges [(id, type, src, dst)]: the types are created in the order they first appear, one bulk insert per type; returns
    the graph and {type: id}"""
    g = host.Graph(hctx, max(n, 1))
    tids = {}
    for t in dict.fromkeys(t for _, t, _, _ in edges):
        tids[t] = g.add_type(t)
        mine = [e for e in edges if e[1] == t]
        g.create_edges(tids[t], [s for _, _, s, _ in mine], [d for _, _, _, d in mine], [i for i, _, _, _ in mine])
    return g, tids


def test_golden_cases_per_row_and_as_one_batch(hctx):
    edges = [(i, t, s, d) for i, (s, t, d) in enumerate(GOLD["graph"]["edges"])]
    g, _ = build(hctx, len(GOLD["graph"]["nodes"]), edges)
    for case in GOLD["cases"]:
        kw = dict(types=tuple(case["types"]), directed=case["directed"], min_hops=case["min_hops"], max_hops=case["max_hops"])
        rows, st = g.shortest_path_batch([r[0] for r in case["rows"]], [r[1] for r in case["rows"]], stats=True, **kw)
        device = sum(1 for s, d, _ in case["rows"] if s != d)
        assert st["device_calls"] == (1 if device else 0), case["name"]
        for (s, d, want), got in zip(case["rows"], rows):
            assert (got[0] if got else None) == want, (case["name"], s, d)
            assert got == g.shortest_path(s, d, **kw), (case["name"], s, d)
            assert got == reference_path(edges, s, d, case["types"], case["directed"], case["min_hops"], case["max_hops"])
    # test01's one evaluated query: a type that does not exist gives Null
    assert g.shortest_path(0, 3, types=("FAKE",)) is None
    assert g.shortest_path_batch([0], [3], types=("FAKE",), stats=True) == ([None], {"device_calls": 0})


def seeded(hctx, seed):
    """a multigraph over types A, B, C; after the commit: relationships added (delta-plus) and deleted (delta-minus), and one
    node deleted with its relationships.  Returns the graph, the node count, the live edge list, the deleted node"""
    rng = random.Random(0x5EED + seed)
    n = rng.randint(12, 40)
    edges = random_multigraph(rng, n, rng.randint(n, 3 * n), ["A", "B", "C"])
    g, tids = build(hctx, n, edges)
    g.commit()
    gone = rng.randrange(n)
    live = []
    for e in edges:                                   # delta-minus: the deleted node's relationships and a few others
        i, t, s, d = e
        if gone in (s, d) or rng.random() < 0.1:
            g.delete_edge(tids[t], s, d, i)
        else:
            live.append(e)
    g.delete_node(gone)
    for k in range(rng.randint(3, 8)):                # delta-plus, onto stored pairs too
        t = rng.choice(["A", "B", "C"])
        s, d = rng.choice([v for v in range(n) if v != gone]), rng.choice([v for v in range(n) if v != gone])
        if live and rng.random() < 0.4:
            _, _, s, d = rng.choice(live)
        if t not in tids:
            continue
        g.create_edge(tids[t], s, d, len(edges) + k)
        live.append((len(edges) + k, t, s, d))
    return g, n, live, gone, list(tids)


def test_batch_equals_row_equals_checker_on_seeded_graphs(hctx):
    found = fallback = multi = one_node = 0
    for seed in range(6):
        g, n, live, gone, graph_types = seeded(hctx, seed)
        rng = random.Random(seed)
        srcs = [rng.randrange(n) for _ in range(24)] + [gone, 0, None, 3, n + 5, 2 ** 40, 1, 1]
        dsts = [rng.randrange(n) for _ in range(24)] + [0, gone, 2, None, 0, 1, n, 1]
        srcs[5] = dsts[5]                               # src == dst among the device's neighbours
        pairs = {}
        for _, _, s, d in live:
            pairs[(s, d)] = pairs.get((s, d), 0) + 1
        for types in ((), ("C", "A"), ("B",), ("A", "nope", "B", "C"), ("nope",)):
            for directed in (True, False):
                for min_hops, max_hops in ((1, None), (0, None), (1, 2)):
                    kw = dict(types=types, directed=directed, min_hops=min_hops, max_hops=max_hops)
                    rows, st = g.shortest_path_batch(srcs, dsts, stats=True, **kw)
                    assert st["device_calls"] == (0 if types == ("nope",) else 1)
                    for s, d, got in zip(srcs, dsts, rows):
                        what = (seed, s, d, kw)
                        assert got == reference_path(live, s, d, list(types), directed, min_hops, max_hops, graph_types), what
                        if (types in ((), ("C", "A")) and max_hops is None) or s is None or d is None:   # (eval_row is slow)
                            assert got == g.shortest_path(s, d, **kw), what
                        if got is None:
                            continue
                        found += 1
                        one_node += len(got[0]) == 1
                        assert len(got[1]) == len(got[0]) - 1      # (every pattern pair has a relationship in a direction)
                        for (u, v), e in zip(zip(got[0], got[0][1:]), got[1]):
                            ends = next((a, b) for i, _, a, b in live if i == e)
                            assert ends in ((u, v), (v, u))
                            fallback += ends != (u, v) and u != v
                            multi += pairs.get((u, v), 0) > 1
    assert found > 300 and fallback > 10 and multi > 10 and one_node > 5


def test_rows_the_device_cannot_take_and_the_error(hctx):
    edges = [(0, "R", 0, 1), (1, "R", 1, 2), (2, "S", 2, 1)]
    g, _ = build(hctx, 4, edges)
    assert g.shortest_path(0, 2) == ([0, 1, 2], [0, 1])
    assert g.shortest_path(0, 2, types=("S",), directed=False) is None
    assert g.shortest_path(1, 2, types=("S",), directed=False) == ([1, 2], [2])   # the (v, u) fallback
    assert g.shortest_path(1, 2, types=("S",)) is None
    assert g.shortest_path(2, 2, min_hops=0) == ([2], []) and g.shortest_path(2, 2) is None
    assert g.shortest_path(None, 2) is None and g.shortest_path(0, None) is None
    # no row qualifies: Null, out of range, src == dst — no device call
    rows, st = g.shortest_path_batch([None, 99, 2, 2 ** 40], [2, 0, 2, 1], min_hops=0, stats=True)
    assert rows == [None, None, ([2], []), None] and st["device_calls"] == 0
    assert g.shortest_path_batch([], [], stats=True) == ([], {"device_calls": 0})
    for bad in ("a string", 1.5, {"v": 1}):
        with pytest.raises(host.HostError, match="A shortestPath requires bound nodes"):
            g.shortest_path(bad, 2)
        with pytest.raises(host.HostError, match="A shortestPath requires bound nodes"):
            g.shortest_path(0, bad)
        with pytest.raises(host.HostError, match="A shortestPath requires bound nodes"):
            g.shortest_path_batch([0, 0], [2, bad])
    assert g.shortest_path(None, "a string") is None   # (the source is looked at first: Null wins)
