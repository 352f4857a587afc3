"""Graph::bulk_insert_edges (host layer over fgpu_edges_build) against its twin loaded with create_edges.  The twins are compared
on EFFECTIVE state — what a reader sees, whatever the fold timing of either path: every edge, every pair's ids, the edge count,
the multi-edge pairs, the adjacency (m \\ dm) U dp, and mt through a transposed traversal."""
import json
import os

import numpy as np
import pytest

from falkordb_amd import _ffi, host

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("device_edges", "fallback_edges", "distinct_pairs", "multi_pairs", "unsorted_runs", "host_sorted_runs")


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def eff_adjacency(g):
    cell = lambda which: {(r, c) for r, c, _ in g.layer(None, which)}
    return (cell("m") - cell("dm")) | cell("dp")


def incoming(g, tname, n):
    """mt of type `tname`: every (dst, src) a transposed CondTraverse over all nodes reaches."""
    nodes = list(range(n))
    rows, nulls, _ = g.cond_traverse_batch(host.cond_spec(hops=[([tname], [])], transposed=True), nodes)
    assert nulls == []
    return sorted((nodes[r], s) for r, s in rows)


def assert_twins(a, b, n, types, probe_pairs):
    """a: the create_edges twin, b: the bulk twin; types = [(type id, name)]."""
    for t, name in types:
        ea, eb = sorted(a.tensor_iter_edges(t)), sorted(b.tensor_iter_edges(t))
        assert ea == eb
        assert a.tensor_edge_count(t) == b.tensor_edge_count(t) == len(ea)
        assert a.tensor_state(t)["multi_pairs"] == b.tensor_state(t)["multi_pairs"]
        for s, d in probe_pairs:
            assert a.tensor_get(t, s, d) == b.tensor_get(t, s, d)
        assert incoming(a, name, n) == incoming(b, name, n) == sorted({(d, s) for s, d, _ in ea})
    assert eff_adjacency(a) == eff_adjacency(b)


def assert_folded(g, t, distinct):
    st = g.tensor_state(t)
    assert st["dp"] == 0 and st["dm"] == 0 and st["m"] == distinct and st["mt"] == distinct


def multigraph(seed, n, m, id0=0, lo=0, hi=None):
    """m edges on nodes [lo, hi): about a quarter repeat a pair, ids id0.. shuffled."""
    rng = np.random.default_rng(seed)
    hi = n if hi is None else hi
    fresh = m - m // 4
    s, d = rng.integers(lo, hi, fresh), rng.integers(lo, hi, fresh)
    again = rng.integers(0, fresh, m - fresh)
    s, d = np.concatenate([s, s[again]]), np.concatenate([d, d[again]])
    mix = rng.permutation(m)
    return s[mix].astype(np.uint64), d[mix].astype(np.uint64), (rng.permutation(m) + id0).astype(np.uint64)


def probes(s, d, n, seed=5):
    rng = np.random.default_rng(seed)
    return sorted({(int(x), int(y)) for x, y in zip(s, d)}) + [(int(x), int(y)) for x, y in rng.integers(0, n, (40, 2))]


def twins(hctx, n, names):
    a, b = host.Graph(hctx, n), host.Graph(hctx, n)
    types = []
    for nm in names:
        t = a.add_type(nm)
        assert b.add_type(nm) == t
        types.append((t, nm))
    return a, b, types


def test_empty_graph_multigraph_batch(hctx):                                   # (a)
    n = 300
    a, b, types = twins(hctx, n, ["R"])
    s, d, ids = multigraph(1, n, 3000)
    a.create_edges(0, s, d, ids)
    st = b.bulk_insert_edges(0, s, d, ids)
    distinct = len(set(zip(s.tolist(), d.tolist())))
    assert tuple(st) == KEYS
    assert st["device_edges"] == 3000 and st["fallback_edges"] == 0 and st["distinct_pairs"] == distinct
    assert st["multi_pairs"] == b.tensor_state(0)["multi_pairs"] > 0 and st["unsorted_runs"] > 0 and st["host_sorted_runs"] == 0
    assert_folded(b, 0, distinct)
    assert eff_adjacency(b) == set(zip(s.tolist(), d.tolist())) and b.layer(None, "dp") == [] and b.layer(None, "dm") == []
    assert_twins(a, b, n, types, probes(s, d, n))
    a.commit(); b.commit()
    assert_twins(a, b, n, types, probes(s, d, n))
    assert b.bulk_insert_edges(0, [], [], []) == dict.fromkeys(KEYS, 0)         # an empty batch does nothing
    assert_folded(b, 0, distinct)


def test_disjoint_second_batch_and_a_second_type(hctx):                        # (b)
    n = 400
    a, b, types = twins(hctx, n, ["R", "S"])
    s1, d1, i1 = multigraph(2, n, 2000, 0, 0, 200)
    s2, d2, i2 = multigraph(3, n, 1500, 2000, 200, 400)                         # no pair in common with the first batch
    s3, d3, i3 = s1[:700], d1[:700], np.arange(5000, 5700, dtype=np.uint64)     # type S shares pairs with type R
    a.create_edges(0, s1, d1, i1)
    b.bulk_insert_edges(0, s1, d1, i1)
    st = b.bulk_insert_edges(0, s2, d2, i2)
    a.create_edges(0, s2, d2, i2)
    assert st["device_edges"] == 1500 and st["fallback_edges"] == 0
    st = b.bulk_insert_edges(1, s3, d3, i3)
    a.create_edges(1, s3, d3, i3)
    assert st["device_edges"] == 700
    pr = set(zip(np.r_[s1, s2].tolist(), np.r_[d1, d2].tolist()))
    assert_folded(b, 0, len(pr))
    assert_folded(b, 1, len(set(zip(s3.tolist(), d3.tolist()))))
    assert eff_adjacency(b) == pr and len(b.layer(None, "m")) == len(pr)        # the union, folded
    assert_twins(a, b, n, types, probes(np.r_[s1, s2], np.r_[d1, d2], n))


def test_colliding_batch_takes_the_edge_by_edge_path(hctx):                    # (c)
    n = 200
    a, b, types = twins(hctx, n, ["R"])
    s1, d1, i1 = multigraph(4, n, 1200)
    a.create_edges(0, s1, d1, i1)
    b.bulk_insert_edges(0, s1, d1, i1)
    s2, d2, i2 = multigraph(5, n, 800, 1200)
    s2[:100], d2[:100] = s1[:100], d1[:100]                                     # singles promoted, multi-edge pairs extended
    a.create_edges(0, s2, d2, i2)
    st = b.bulk_insert_edges(0, s2, d2, i2)
    assert st["fallback_edges"] == 800 and st["device_edges"] == 0
    assert_twins(a, b, n, types, probes(np.r_[s1, s2], np.r_[d1, d2], n))
    a.commit(); b.commit()
    assert_twins(a, b, n, types, probes(np.r_[s1, s2], np.r_[d1, d2], n))


def test_edits_after_a_bulk_load(hctx):                                        # (d)
    n = 50
    a, b, types = twins(hctx, n, ["R"])
    s = np.array([1, 1, 2, 3, 3, 3, 7], dtype=np.uint64)
    d = np.array([2, 2, 4, 5, 5, 5, 7], dtype=np.uint64)
    ids = np.array([11, 10, 20, 32, 30, 31, 40], dtype=np.uint64)
    a.create_edges(0, s, d, ids)
    assert b.bulk_insert_edges(0, s, d, ids)["multi_pairs"] == 2
    pp = probes(s, d, n)
    for g in (a, b):
        g.delete_edge(0, 1, 2, 10)          # a 2-edge pair demotes: 11 returns inline
    assert b.tensor_get(0, 1, 2) == [11] and b.tensor_state(0)["multi_pairs"] == 1
    assert_twins(a, b, n, types, pp)
    for g in (a, b):
        g.create_edge(0, 2, 4, 21)          # a single pair promotes
    assert b.tensor_get(0, 2, 4) == [20, 21]
    assert_twins(a, b, n, types, pp)
    for g in (a, b):
        g.delete_edge(0, 7, 7, 40)          # a pair empties: it leaves the adjacency and mt
    assert b.tensor_get(0, 7, 7) == [] and (7, 7) not in eff_adjacency(b)
    assert_twins(a, b, n, types, pp)
    for g in (a, b):
        g.commit()
    assert_twins(a, b, n, types, pp)
    assert b.tensor_edge_count(0) == 6


def test_social_fixture_loaded_in_bulk(hctx):                                  # (e): tests/test_gpu_host.py test_social_queries' calls
    with open(os.path.join(GOLD, "social.json")) as f:
        s = json.load(f)
    names = [p["name"] for p in s["persons"]] + s["countries"]
    ids = {nm: i for i, nm in enumerate(names)}
    g = host.Graph(hctx, len(names))
    lp, lc = g.add_label("person"), g.add_label("country")
    for p in s["persons"]:
        g.label_node(ids[p["name"]], lp)
    for c in s["countries"]:
        g.label_node(ids[c], lc)
    tf, tv = g.add_type("friend"), g.add_type("visited")
    nv = len(s["visits"])
    st = g.bulk_insert_edges(tv, [ids[a] for a, _, _ in s["visits"]], [ids[b] for _, b, _ in s["visits"]], np.arange(nv))
    assert st["device_edges"] == nv
    st = g.bulk_insert_edges(tf, [ids[a] for a, _ in s["friends"]], [ids[b] for _, b in s["friends"]],
                             np.arange(nv, nv + len(s["friends"])))
    assert st["device_edges"] == len(s["friends"])
    roi = ids["Roi Lipman"]
    rows, nulls, _ = g.cond_traverse_batch(host.cond_spec(src_labels=["person"], hops=[(["friend"], ["person"])]), [roi])
    assert sorted(names[d] for _, d in rows) == sorted(r[0] for r in s["queries"]["my_friends_query"]["expected"])
    rows2, _, _ = g.cond_traverse_batch(host.cond_spec(hops=[(["friend"], ["person"])]), [d for _, d in rows])
    fof = [names[d] for _, d in rows2]
    assert sorted(fof) == sorted(r[0] for r in s["queries"]["friends_of_friends_query"]["expected"])
    fused = host.cond_spec(src_labels=["person"], hops=[(["friend"], []), (["friend"], ["person"])])
    rows3, _, flops = g.cond_traverse_batch(fused, [roi])
    assert sorted(names[d] for _, d in rows3) == sorted(set(fof)) and flops > 0
    attrs = {p["name"]: p for p in s["persons"]}
    singles = [ids[nm] for nm in fof if attrs[nm]["status"] == "single"]
    rows4, _, _ = g.cond_traverse_batch(host.cond_spec(hops=[(["visited"], ["country"])]), singles)
    got = sorted({names[singles[i]] for i, d in rows4 if names[d] == "Netherlands"})
    assert got == [r[0] for r in s["queries"]["friends_of_friends_visited_netherlands_and_single_query"]["expected"]]
    want = dict(map(tuple, s["queries"]["relation_type_counts"]["expected"]))
    assert g.tensor_edge_count(tf) == want["friend"] and g.tensor_edge_count(tv) == want["visited"]


def test_a_matrix_built_before_a_bulk_insert_is_unchanged(hctx):               # (f)
    n = 300
    g = host.Graph(hctx, n)
    g.add_type("R")
    s1, d1, i1 = multigraph(6, n, 1500, 0, 0, 150)
    g.bulk_insert_edges(0, s1, d1, i1)
    g.create_edge(0, 299, 298, 9000)                                            # ... and a pending delta beside the base
    snaps = [g.build_adjacency([]), g.build_adjacency(["R"])]
    before = [sorted(m.iter()) for m in snaps]
    assert len(before[0]) == len(set(zip(s1.tolist(), d1.tolist()))) + 1
    s2, d2, i2 = multigraph(7, n, 1000, 1500, 150, 290)
    assert g.bulk_insert_edges(0, s2, d2, i2)["device_edges"] == 1000
    assert [sorted(m.iter()) for m in snaps] == before
    assert len(g.build_adjacency([]).iter()) == len(before[0]) + len(set(zip(s2.tolist(), d2.tolist())))
    assert g.tensor_get(0, 299, 298) == [9000]                                  # the folded delta is still there


@pytest.mark.parametrize("bad", ["source", "marker", "triple"])
def test_a_rejected_batch_leaves_the_graph_as_it_was(hctx, bad):               # (g)
    n = 100
    g = host.Graph(hctx, n)
    g.add_type("R")
    s1, d1, i1 = multigraph(8, n, 500)
    g.bulk_insert_edges(0, s1, d1, i1)
    g.create_edge(0, 3, 4, 7000)
    edges, count, adj, state = sorted(g.tensor_iter_edges(0)), g.tensor_edge_count(0), eff_adjacency(g), g.tensor_state(0)
    s, d, ids = [1, n, 2], [2, 3, 4], [9001, 9002, 9003]                        # a source at the capacity
    if bad == "marker":
        s, ids = [1, 5, 2], [9001, 2**64 - 1, 9003]
    elif bad == "triple":
        s, ids = [1, 1, 1], [9001, 9002, 9001]
        d = [2, 2, 2]
    with pytest.raises(host.HostError) as e:
        g.bulk_insert_edges(0, s, d, ids)
    assert e.value.code == _ffi.FGPU_INVALID
    assert sorted(g.tensor_iter_edges(0)) == edges and g.tensor_edge_count(0) == count == 501
    assert eff_adjacency(g) == adj and g.tensor_state(0) == state
    assert g.bulk_insert_edges(0, [n - 1], [n - 1], [9100])["device_edges"] in (0, 1)   # and the graph goes on working
    assert g.tensor_edge_count(0) == 502
