"""Graph::append_edges_bulk (host layer over fgpu_edges_build + fgpu_edges_union) against its twin fed with create_edges, in the
manner of tests/test_gpu_bulk_insert_host.py.  The twins are compared on EFFECTIVE state — what a reader sees, whatever the fold
timing of either path: every edge, every pair's ids, the edge count, the multi-edge pairs, the adjacency (m \\ dm) U dp, and mt
through a transposed traversal — before and after commit."""
import numpy as np
import pytest

from falkordb_amd import _ffi, host

pytestmark = pytest.mark.gpu

KEYS = ("edges", "distinct_pairs", "multi_pairs", "colliding_pairs", "promoted_pairs", "extended_pairs", "me_rows", "host_sorted_runs")


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
    """a: the create_edges twin, b: the append twin; types = [(type id, name)]."""
    for t, name in types:
        ea, eb = sorted(a.tensor_iter_edges(t)), sorted(b.tensor_iter_edges(t))
        assert ea == eb
        assert a.tensor_edge_count(t) == b.tensor_edge_count(t) == len(ea)
        assert a.tensor_state(t)["multi_pairs"] == b.tensor_state(t)["multi_pairs"]
        for s, d in probe_pairs:
            assert a.tensor_get(t, s, d) == b.tensor_get(t, s, d)
        assert incoming(a, name, n) == incoming(b, name, n) == sorted({(d, s) for s, d, _ in ea})
    assert eff_adjacency(a) == eff_adjacency(b)


def assert_folded(g, t):
    st = g.tensor_state(t)
    distinct = len({(s, d) for s, d, _ in g.tensor_iter_edges(t)})
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


def test_a_colliding_batch_goes_through_the_device(hctx):
    """The batch of test_colliding_batch_takes_the_edge_by_edge_path: singles promoted, multi-edge pairs extended, new pairs."""
    n = 200
    a, b, types = twins(hctx, n, ["R"])
    s1, d1, i1 = multigraph(4, n, 1200)
    a.create_edges(0, s1, d1, i1)
    b.bulk_insert_edges(0, s1, d1, i1)
    s2, d2, i2 = multigraph(5, n, 800, 1200)
    s2[:100], d2[:100] = s1[:100], d1[:100]
    a.create_edges(0, s2, d2, i2)
    st = b.append_edges_bulk(0, s2, d2, i2)
    assert tuple(st) == KEYS
    assert st["edges"] == 800 and st["distinct_pairs"] == len(set(zip(s2.tolist(), d2.tolist())))
    assert st["colliding_pairs"] == st["promoted_pairs"] + st["extended_pairs"] and st["promoted_pairs"] > 0 and st["extended_pairs"] > 0
    assert st["colliding_pairs"] == len(set(zip(s1.tolist(), d1.tolist())) & set(zip(s2.tolist(), d2.tolist())))
    assert st["me_rows"] >= st["colliding_pairs"]
    assert_folded(b, 0)
    assert b.layer(None, "dp") == [] and b.layer(None, "dm") == []
    pp = probes(np.r_[s1, s2], np.r_[d1, d2], n)
    assert_twins(a, b, n, types, pp)
    a.commit(); b.commit()
    assert_twins(a, b, n, types, pp)


@pytest.mark.parametrize("pairs, dup", [(64, 2), (1000, 2), (1000, 3), (5000, 2)])
def test_dup_rounds_of_the_same_pairs_as_separate_batches(hctx, pairs, dup):
    """tensor.rs:1386-1425 (multi_pairs_matches_the_sentinel_count): `dup` edges on every pair (i, i + 1), one batch a round.
    The first round loads an empty tensor, the second promotes every pair, the third extends every row."""
    n = pairs + 1
    g = host.Graph(hctx, n)
    g.add_type("R")
    srcs = np.arange(pairs, dtype=np.uint64)
    for rnd in range(dup):
        st = g.append_edges_bulk(0, srcs, srcs + np.uint64(1), srcs + np.uint64(rnd * pairs))
        assert st["colliding_pairs"] == (pairs if rnd else 0)
        assert (st["promoted_pairs"], st["extended_pairs"]) == {0: (0, 0), 1: (pairs, 0), 2: (0, pairs)}[rnd]
    state = g.tensor_state(0)
    assert state["multi_pairs"] == pairs and state["m"] == pairs and state["dp"] == 0 and state["dm"] == 0
    assert g.tensor_edge_count(0) == pairs * dup
    assert sum(1 for _, _, v in g.layer(0, "m") if v == 2**64 - 1) == pairs              # the sentinel count
    for i in (0, pairs // 2, pairs - 1):
        assert g.tensor_get(0, i, i + 1) == [r * pairs + i for r in range(dup)]
    g.commit()
    assert g.tensor_edge_count(0) == pairs * dup and g.tensor_state(0)["multi_pairs"] == pairs


def test_pending_deltas_are_folded_first_and_survive(hctx):
    n = 60
    a, b, types = twins(hctx, n, ["R"])
    s = np.array([1, 1, 2, 3, 3, 3, 7, 8], dtype=np.uint64)
    d = np.array([2, 2, 4, 5, 5, 5, 7, 9], dtype=np.uint64)
    ids = np.array([11, 10, 20, 32, 30, 31, 40, 50], dtype=np.uint64)
    a.create_edges(0, s, d, ids)
    b.bulk_insert_edges(0, s, d, ids)
    for g in (a, b):
        g.create_edge(0, 20, 21, 60)        # a pending new pair
        g.create_edge(0, 2, 4, 21)          # a pending promotion
        g.delete_edge(0, 1, 2, 10)          # a 2-edge pair demotes: 11 returns inline
        g.delete_edge(0, 7, 7, 40)          # a pair empties
    assert b.tensor_state(0)["dp"] > 0 and b.tensor_state(0)["dm"] > 0
    # the batch lands on every one of them: the demoted pair is promoted again, the emptied pair is new again
    s2 = np.array([20, 2, 1, 7, 8, 30, 30], dtype=np.uint64)
    d2 = np.array([21, 4, 2, 7, 9, 31, 31], dtype=np.uint64)
    i2 = np.array([61, 22, 12, 41, 51, 70, 71], dtype=np.uint64)
    a.create_edges(0, s2, d2, i2)
    st = b.append_edges_bulk(0, s2, d2, i2)
    assert (st["colliding_pairs"], st["promoted_pairs"], st["extended_pairs"], st["multi_pairs"]) == (4, 3, 1, 1)
    assert_folded(b, 0)
    assert b.tensor_get(0, 20, 21) == [60, 61] and b.tensor_get(0, 2, 4) == [20, 21, 22] and b.tensor_get(0, 1, 2) == [11, 12]
    assert b.tensor_get(0, 7, 7) == [41] and b.tensor_get(0, 8, 9) == [50, 51] and b.tensor_get(0, 30, 31) == [70, 71]
    pp = probes(np.r_[s, s2], np.r_[d, d2], n)
    assert_twins(a, b, n, types, pp)
    a.commit(); b.commit()
    assert_twins(a, b, n, types, pp)


def test_a_second_type_sharing_pairs(hctx):
    n = 300
    a, b, types = twins(hctx, n, ["R", "S"])
    s1, d1, i1 = multigraph(2, n, 2000, 0, 0, 200)
    s2, d2, i2 = multigraph(3, n, 1500, 2000, 100, 300)                          # shares the nodes [100, 200) with the first
    s3, d3, i3 = np.r_[s1[:700], s2[:300]], np.r_[d1[:700], d2[:300]], np.arange(5000, 6000, dtype=np.uint64)
    for g, load in ((a, a.create_edges), (b, b.append_edges_bulk)):
        load(0, s1, d1, i1)
        load(1, s3, d3, i3)
        load(0, s2, d2, i2)
        load(1, s2[200:900], d2[200:900], np.arange(7000, 7700, dtype=np.uint64))
    pr = set(zip(np.r_[s1, s2].tolist(), np.r_[d1, d2].tolist()))
    assert_folded(b, 0)
    assert_folded(b, 1)
    assert eff_adjacency(b) == pr and len(b.layer(None, "m")) == len(pr)          # the union, folded
    pp = probes(np.r_[s1, s2], np.r_[d1, d2], n)
    assert_twins(a, b, n, types, pp)
    a.commit(); b.commit()
    assert_twins(a, b, n, types, pp)


def test_a_matrix_built_before_the_call_is_unchanged(hctx):
    n = 300
    g = host.Graph(hctx, n)
    g.add_type("R")
    s1, d1, i1 = multigraph(6, n, 1500, 0, 0, 150)
    g.append_edges_bulk(0, s1, d1, i1)
    g.create_edge(0, 299, 298, 9000)                                            # ... and a pending delta beside the base
    snaps = [g.build_adjacency([]), g.build_adjacency(["R"])]
    before = [sorted(m.iter()) for m in snaps]
    assert len(before[0]) == len(set(zip(s1.tolist(), d1.tolist()))) + 1
    s2, d2, i2 = multigraph(7, n, 1000, 1500, 100, 290)                         # collides with the loaded pairs on [100, 150)
    st = g.append_edges_bulk(0, s2, d2, i2)
    assert st["edges"] == 1000
    assert [sorted(m.iter()) for m in snaps] == before
    assert len(g.build_adjacency([]).iter()) == len(set(zip(np.r_[s1, s2].tolist(), np.r_[d1, d2].tolist()))) + 1
    assert g.tensor_get(0, 299, 298) == [9000]                                  # the folded delta is still there


def test_an_empty_batch_and_an_empty_tensor(hctx):
    n = 100
    a, b, types = twins(hctx, n, ["R"])
    assert b.append_edges_bulk(0, [], [], []) == dict.fromkeys(KEYS, 0)         # nothing onto nothing
    assert b.tensor_state(0) == a.tensor_state(0)
    s, d, ids = multigraph(9, n, 600)
    a.create_edges(0, s, d, ids)
    st = b.append_edges_bulk(0, s, d, ids)                                      # an empty tensor adopts the pieces
    assert st["edges"] == 600 and st["colliding_pairs"] == 0 and st["me_rows"] == st["multi_pairs"] > 0
    assert_folded(b, 0)
    state = b.tensor_state(0)
    assert b.append_edges_bulk(0, [], [], []) == dict.fromkeys(KEYS, 0)         # an empty batch does nothing
    assert b.tensor_state(0) == state
    assert_twins(a, b, n, types, probes(s, d, n))


@pytest.mark.parametrize("bad", ["stored-inline", "stored-in-a-row", "source", "marker", "triple"])
def test_a_rejected_batch_leaves_the_graph_as_it_was(hctx, bad):
    n = 100
    g = host.Graph(hctx, n)
    g.add_type("R")
    s1, d1, i1 = multigraph(8, n, 500)
    g.append_edges_bulk(0, s1, d1, i1)
    if not bad.startswith("stored"):
        g.create_edge(0, 3, 4, 7000)       # (the build rejects before the layers are folded: a pending delta stays pending)
    edges = sorted(g.tensor_iter_edges(0))
    count, adj, state = g.tensor_edge_count(0), eff_adjacency(g), g.tensor_state(0)
    inline = next((s, d, i) for s, d, i in edges if len(g.tensor_get(0, s, d)) == 1)
    in_row = next((s, d, i) for s, d, i in edges if len(g.tensor_get(0, s, d)) > 1)
    s, d, ids = {
        "stored-inline": ([1, inline[0], 2], [2, inline[1], 4], [9001, inline[2], 9003]),
        "stored-in-a-row": ([1, in_row[0], in_row[0]], [2, in_row[1], in_row[1]], [9001, in_row[2], 9003]),
        "source": ([1, n, 2], [2, 3, 4], [9001, 9002, 9003]),                   # a source at the capacity
        "marker": ([1, 5, 2], [2, 3, 4], [9001, 2**64 - 1, 9003]),
        "triple": ([1, 1, 1], [2, 2, 2], [9001, 9002, 9001]),
    }[bad]
    with pytest.raises(host.HostError) as e:
        g.append_edges_bulk(0, s, d, ids)
    assert e.value.code == _ffi.FGPU_INVALID
    assert sorted(g.tensor_iter_edges(0)) == edges and g.tensor_edge_count(0) == count
    assert eff_adjacency(g) == adj and g.tensor_state(0) == state
    assert g.append_edges_bulk(0, [n - 1, inline[0]], [n - 1, inline[1]], [9100, 9101])["edges"] == 2   # the graph goes on working
    assert g.tensor_edge_count(0) == count + 2 and g.tensor_get(0, inline[0], inline[1]) == sorted([inline[2], 9101])


def test_a_round_trip_through_delete_edges_bulk(hctx):
    """The appended edges deleted in bulk: the graph is back at the state of a twin that never saw them."""
    n = 200
    a, b, types = twins(hctx, n, ["R"])
    s1, d1, i1 = multigraph(4, n, 1200)
    for g in (a, b):
        g.bulk_insert_edges(0, s1, d1, i1)
    s2, d2, i2 = multigraph(5, n, 800, 1200)
    s2[:100], d2[:100] = s1[:100], d1[:100]
    st = b.append_edges_bulk(0, s2, d2, i2)
    assert st["promoted_pairs"] > 0 and st["extended_pairs"] > 0
    assert b.tensor_edge_count(0) == 2000
    rels = b.delete_edges_bulk(0, s2, d2, i2)
    assert sorted(rels) == sorted(zip(i2.tolist(), s2.tolist(), d2.tolist()))
    pp = probes(np.r_[s1, s2], np.r_[d1, d2], n)
    assert_twins(a, b, n, types, pp)
    assert b.tensor_state(0) == a.tensor_state(0)
    a.commit(); b.commit()
    assert_twins(a, b, n, types, pp)
