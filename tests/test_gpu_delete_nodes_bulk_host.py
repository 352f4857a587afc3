"""Graph::delete_nodes_bulk (host layer over fgpu_nodes_detach) against its twin, which deletes through the API that existed
before it: one delete_edge per incident edge collected from tensor_iter_edges, then delete_node.  As in
tests/test_gpu_bulk_insert_host.py the twins are compared on EFFECTIVE state — every edge, every pair's ids, the edge counts, the
multi-edge pairs, mt through a transposed traversal, the adjacency (m \\ dm) U dp — and the returned list is held against
tests/detach_check.py, in order."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detach_check import delete_nodes  # noqa: E402

pytestmark = pytest.mark.gpu

N = 320
TYPES = [(0, "R"), (1, "S")]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def eff_adjacency(g):
    cell = lambda which: {(r, c) for r, c, _ in g.layer(None, which)}
    return (cell("m") - cell("dm")) | cell("dp")


def incoming(g, tname, n):
    nodes = list(range(n))
    rows, nulls, _ = g.cond_traverse_batch(host.cond_spec(hops=[([tname], [])], transposed=True), nodes)
    assert nulls == []
    return sorted((nodes[r], s) for r, s in rows)


def assert_twins(a, b, probe_pairs):
    for t, name in TYPES:
        ea, eb = sorted(a.tensor_iter_edges(t)), sorted(b.tensor_iter_edges(t))
        assert ea == eb
        assert a.tensor_edge_count(t) == b.tensor_edge_count(t) == len(ea)
        assert a.tensor_state(t)["multi_pairs"] == b.tensor_state(t)["multi_pairs"]
        for s, d in probe_pairs:
            assert a.tensor_get(t, s, d) == b.tensor_get(t, s, d)
        assert incoming(a, name, N) == incoming(b, name, N) == sorted({(d, s) for s, d, _ in ea})
    assert eff_adjacency(a) == eff_adjacency(b)


def multigraph(seed, n, m, id0=0):
    """m edges on the nodes below n - 4 (the last four have none): about a quarter repeat a pair, a few are self-loops, ids
    id0.. shuffled."""
    rng = np.random.default_rng(seed)
    fresh = m - m // 4
    s, d = rng.integers(0, n - 4, fresh), rng.integers(0, n - 4, fresh)
    d[:12] = s[:12]
    again = rng.integers(0, fresh, m - fresh)
    s, d = np.concatenate([s, s[again]]), np.concatenate([d, d[again]])
    mix = rng.permutation(m)
    return s[mix].astype(np.uint64), d[mix].astype(np.uint64), (rng.permutation(m) + id0).astype(np.uint64)


def make_twins(hctx, seed=11, labels=True):
    """Twin graphs: type R a multigraph of 1200 edges, type S 500 edges of which 300 share R's pairs; labels on a third of the
    nodes.  Returns (a, b, edges_by_type, label pairs)."""
    a, b = host.Graph(hctx, N), host.Graph(hctx, N)
    s1, d1, i1 = multigraph(seed, N, 1200)
    s2, d2, i2 = multigraph(seed + 1, N, 200, 5000)
    s2, d2 = np.r_[s1[:300], s2], np.r_[d1[:300], d2]
    i2 = np.r_[np.arange(4000, 4300, dtype=np.uint64), i2]
    lab = []
    for g in (a, b):
        for _, nm in TYPES:
            g.add_type(nm)
        g.bulk_insert_edges(0, s1, d1, i1)
        g.bulk_insert_edges(1, s2, d2, i2)
        if labels:
            l0, l1 = g.add_label("L0"), g.add_label("L1")
            lab = [(v, l0) for v in range(0, N, 3)] + [(v, l1) for v in range(0, N, 7)]
            for v, l in lab:
                g.label_node(v, l)
            g.commit()
    by_type = [list(zip(s1.tolist(), d1.tolist(), i1.tolist())), list(zip(s2.tolist(), d2.tolist(), i2.tolist()))]
    return a, b, by_type, lab


def pick_nodes(by_type, k=18, seed=3):
    """k nodes: both ends of one edge of a multi-edge pair, one node with a self-loop, the last node, the rest random."""
    rng = np.random.default_rng(seed)
    seen, multi = set(), None
    for s, d, _ in by_type[0]:
        if (s, d) in seen and s != d:
            multi = (s, d)
            break
        seen.add((s, d))
    loop = next(s for s, d, _ in by_type[0] if s == d)
    D = {multi[0], multi[1], loop, N - 1}
    while len(D) < k:
        D.add(int(rng.integers(0, N)))
    return sorted(D)


def edge_by_edge(g, D):
    """Today's path: every edge incident to D, collected from tensor_iter_edges, through delete_edge; then delete_node."""
    Ds = set(D)
    for t, _ in TYPES:
        for s, d, i in g.tensor_iter_edges(t):
            if s in Ds or d in Ds:
                g.delete_edge(t, s, d, i)
    for v in D:
        g.delete_node(v)


def probes(by_type, D):
    Ds = set(D)
    inc = sorted({(s, d) for es in by_type for s, d, _ in es if s in Ds or d in Ds})
    rest = sorted({(s, d) for es in by_type for s, d, _ in es} - set(inc))
    return inc[:60] + rest[:40]


def assert_folded(g, want):
    for t, _ in TYPES:
        st = g.tensor_state(t)
        pairs = len({(s, d) for s, d, _ in want["edges"][t]})
        assert st["dp"] == 0 and st["dm"] == 0 and st["m"] == pairs and st["mt"] == pairs
        assert sorted(g.tensor_iter_edges(t)) == want["edges"][t]


def test_twins_agree_and_the_list_is_the_reference_s(hctx):
    a, b, by_type, lab = make_twins(hctx)
    D = pick_nodes(by_type)
    want = delete_nodes(by_type, D, labels=lab)
    pp = probes(by_type, D)
    version = [b.tensor_version(t) for t, _ in TYPES]                      # a reader's version, taken before the delete
    built = b.build_adjacency([])
    built_before = sorted(built.iter())
    edge_by_edge(a, D)
    messy = np.random.default_rng(1).permutation(np.r_[D, D[:5]])          # any order, duplicates allowed
    rels, st = b.delete_nodes_bulk(messy, stats=True)
    assert rels == want["list"]
    removed = sum(len(es) for es in by_type) - sum(len(es) for es in want["edges"])
    assert st["nodes"] == len(D) and st["edges_removed"] == st["edges_listed"] == removed == len(rels)
    assert st["label_entries"] == len(lab) - len(want["labels"]) and st["multi_pairs"] > 0
    assert st["adjacency_entries"] == len({(s, d) for es in by_type for s, d, _ in es}) - len(want["adjacency"])
    assert_twins(a, b, pp)
    assert_folded(b, want)
    assert eff_adjacency(b) == want["adjacency"] and b.layer(None, "dp") == [] and b.layer(None, "dm") == []
    # the node x label matrix lost the rows of D and nothing else
    left = set(want["labels"])
    for v, l in lab[::4] + [(v, l) for v, l in lab if v in set(D)]:
        assert b.node_has_label(v, l) == ((v, l) in left)
    # the version taken before still sees every edge, and so does the matrix built before
    for t, _ in TYPES:
        ids = {}
        for s, d, i in by_type[t]:
            ids.setdefault((s, d), []).append(i)
        assert version[t].state()["edge_count"] == len(by_type[t])
        for s, d in pp:
            assert version[t].get(s, d) == sorted(ids.get((s, d), []))
    assert sorted(built.iter()) == built_before
    # a second delete of the same nodes finds nothing
    state = [b.tensor_state(t) for t, _ in TYPES]
    rels2, st2 = b.delete_nodes_bulk(D, stats=True)
    assert rels2 == [] and st2["edges_removed"] == st2["label_entries"] == st2["adjacency_entries"] == 0
    assert [b.tensor_state(t) for t, _ in TYPES] == state
    assert_twins(a, b, pp)
    a.commit(); b.commit()
    assert_twins(a, b, pp)
    assert_folded(b, want)


def test_skipped_ids_leave_the_list_but_not_the_graph_alone(hctx):
    a, b, by_type, _ = make_twins(hctx, seed=21, labels=False)
    D = pick_nodes(by_type, k=12, seed=4)
    full = delete_nodes(by_type, D)["list"]
    skip = [i for i, _, _ in full[::3]]
    want = delete_nodes(by_type, D, skip_ids=skip)
    assert 0 < len(want["list"]) < len(full)
    edge_by_edge(a, D)
    rels, st = b.delete_nodes_bulk(D, skip_ids=skip, stats=True)
    assert rels == want["list"] and st["edges_listed"] == len(rels) and st["edges_removed"] == len(full)
    assert_twins(a, b, probes(by_type, D))
    assert_folded(b, want)
    i, s, d = full[0]                                                       # the explicit delete that follows finds the pair absent
    t = 0 if (s, d, i) in set(by_type[0]) else 1
    b.delete_edge(t, s, d, i)
    assert_folded(b, want)


def test_unfolded_deltas_before_the_call(hctx):
    """Edges created and deleted edge by edge, with no commit, leave dp and dm populated: the call folds them first."""
    a, b, by_type, _ = make_twins(hctx, seed=31, labels=False)
    D = pick_nodes(by_type, k=12, seed=5)
    p, q = [v for v in range(200, N) if v not in D][:2]                     # two nodes that stay
    extra = [(D[0], 7, 9000), (8, D[1], 9001), (D[2], D[3], 9002), (p, q, 9003), (D[0], 7, 9004)]
    gone = by_type[0][:25]
    for g in (a, b):
        for s, d, i in extra:
            g.create_edge(0, s, d, i)
        for s, d, i in gone:
            g.delete_edge(0, s, d, i)
    st = b.tensor_state(0)
    assert st["dp"] > 0 and st["dm"] > 0
    by_type[0] = by_type[0][25:] + extra
    want = delete_nodes(by_type, D)
    edge_by_edge(a, D)
    assert b.delete_nodes_bulk(D) == want["list"]
    assert_twins(a, b, probes(by_type, D))
    assert_folded(b, want)
    assert 9003 in b.tensor_get(0, p, q)                                   # the folded delta is still there


def test_vector_indexes_lose_the_deleted_nodes_and_edges(hctx):
    g = host.Graph(hctx, 40)
    person, knows = g.add_label("Person"), g.add_type("Knows")
    g.vector_index_create(False, person, "emb", 2, "euclidean")
    g.vector_index_create(True, knows, "emb", 2, None)
    s, d = np.arange(30, dtype=np.uint64), (np.arange(30, dtype=np.uint64) + 1) % 30
    g.bulk_insert_edges(knows, s, d, np.arange(100, 130, dtype=np.uint64))
    for v in range(30):
        g.label_node(v, person)
        g.vector_set_node(person, "emb", v, [v, 0])
        g.vector_set_edge(knows, "emb", v, (v + 1) % 30, 100 + v, [v, 1])
    rels = g.delete_nodes_bulk([5, 6, 20], skip_ids=[105])
    assert sorted(i for i, _, _ in rels) == [104, 106, 119, 120]           # 105 = 5->6 is skipped, and gone all the same
    nodes, _ = g.vector_query_nodes("Person", "emb", 100, [0, 0])
    assert sorted(nodes.tolist()) == [v for v in range(30) if v not in (5, 6, 20)]
    edges, _, _, _ = g.vector_query_edges("Knows", "emb", 100, [0, 0])
    assert sorted(edges.tolist()) == [100 + v for v in range(30) if v not in (4, 5, 6, 19, 20)]


def test_nothing_to_do_and_a_node_past_the_capacity(hctx):
    a, b, by_type, lab = make_twins(hctx, seed=41)
    state = [b.tensor_state(t) for t, _ in TYPES]
    adj = eff_adjacency(b)
    rels, st = b.delete_nodes_bulk([], stats=True)
    assert rels == [] and set(st.values()) == {0}
    with pytest.raises(host.HostError) as e:
        b.delete_nodes_bulk([3, N, 4])
    assert e.value.code == _ffi.FGPU_INVALID
    assert [b.tensor_state(t) for t, _ in TYPES] == state and eff_adjacency(b) == adj
    assert b.node_has_label(3, 0)                                          # node 3 kept its label: nothing ran
    rels, st = b.delete_nodes_bulk([N - 2, N - 3], stats=True)             # nodes without edges: only their labels go
    assert rels == [] and st["nodes"] == 2 and st["edges_removed"] == 0 and st["adjacency_entries"] == 0
    assert st["label_entries"] == sum(1 for v, _ in lab if v in (N - 2, N - 3)) > 0
    assert [b.tensor_state(t) for t, _ in TYPES] == state
    assert_twins(a, b, probes(by_type, [0]))                               # (twin a was never touched)
