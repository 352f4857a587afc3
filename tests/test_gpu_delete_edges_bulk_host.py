"""Graph::delete_edges_bulk (host layer over fgpu_edges_remove) against its twin, which deletes through the API that existed
before it: one delete_edge per edge.  The twins are those of tests/test_gpu_delete_nodes_bulk_host.py — N = 320, types R and S
sharing pairs, multi-edges, self-loops — and are compared on EFFECTIVE state with its assert_twins: every edge, every pair's ids,
the edge counts, the multi-edge pairs, mt through a transposed traversal, the adjacency.  The returned list is held against
tests/edges_remove_check.py."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edges_remove_check import delete_edges  # noqa: E402
from test_gpu_delete_nodes_bulk_host import N, TYPES, assert_twins, eff_adjacency, make_twins, pick_nodes  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def ids_of(by_type):
    """per type: {(src, dst): ascending ids}"""
    out = []
    for es in by_type:
        d = {}
        for s, dd, i in es:
            d.setdefault((s, dd), []).append(i)
        out.append({k: sorted(v) for k, v in d.items()})
    return out


def edge_by_edge(g, batch):
    for t, s, d, i in batch:
        g.delete_edge(t, s, d, i)


def bulk(g, batch, **kw):
    t, s, d, i = (np.array([b[k] for b in batch], dtype=np.uint64) for k in range(4))
    return g.delete_edges_bulk(t, s, d, i, **kw)


def assert_state(g, want):
    """the tensors hold want['edges'], folded, and the adjacency is want['adjacency'] in effect"""
    for t, _ in TYPES:
        st = g.tensor_state(t)
        pairs = ids_of([want["edges"][t]])[0]
        assert st["dp"] == 0 and st["dm"] == 0 and st["m"] == len(pairs) and st["mt"] == len(pairs)
        assert sorted(g.tensor_iter_edges(t)) == want["edges"][t]
        assert st["multi_pairs"] == sum(1 for v in pairs.values() if len(v) > 1)
    assert eff_adjacency(g) == want["adjacency"]


def probes_of(by_type, batch):
    touched = sorted({(s, d) for _, s, d, _ in batch})
    rest = sorted({(s, d) for es in by_type for s, d, _ in es} - set(touched))
    return touched[:80] + rest[:40]


def test_twins_agree_and_the_list_is_the_checker_s(hctx):
    """A seeded tenth of the edges of both types, shuffled, with a few repeated and a few that name nothing."""
    a, b, by_type, _ = make_twins(hctx, labels=False)
    rng = np.random.default_rng(5)
    real = [(t, s, d, i) for t, _ in TYPES for s, d, i in by_type[t]]
    batch = [real[k] for k in rng.choice(len(real), len(real) // 10, replace=False)]
    noise = [(0, 1, 2, 999999), (1, batch[0][1], batch[0][2], 999998), (0, N - 1, N - 1, 5), batch[3], batch[7]]
    want = delete_edges(by_type, batch + noise)
    version = [b.tensor_version(t) for t, _ in TYPES]                      # a reader's version, taken before the delete
    edge_by_edge(a, batch)
    messy = [(batch + noise)[k] for k in rng.permutation(len(batch) + len(noise))]
    rels, st = bulk(b, messy, stats=True)
    assert rels == delete_edges(by_type, messy)["list"] and sorted(rels) == sorted(want["list"])
    assert st["edges_named"] == len(messy) and st["edges_removed"] == len(batch) == len(rels)
    assert st["per_type"] == [sum(1 for x in batch if x[0] == t) for t, _ in TYPES]
    all_pairs = {(s, d) for es in by_type for s, d, _ in es}
    assert st["adjacency_entries"] == len(all_pairs) - len(want["adjacency"]) > 0
    assert st["pairs_emptied"] >= st["adjacency_entries"]
    pp = probes_of(by_type, batch)
    assert_twins(a, b, pp)
    assert_state(b, want)
    before = ids_of(by_type)
    for t, _ in TYPES:                                                     # the version taken before still sees every edge
        assert version[t].state()["edge_count"] == len(by_type[t])
        for s, d in pp:
            assert version[t].get(s, d) == before[t].get((s, d), [])
    rels2, st2 = bulk(b, messy, stats=True)                                # a second delete of the same edges finds nothing
    assert rels2 == [] and st2["edges_removed"] == st2["pairs_emptied"] == st2["adjacency_entries"] == 0
    assert_state(b, want)
    a.commit(); b.commit()
    assert_twins(a, b, pp)
    assert_state(b, want)


def test_multi_edge_pairs_demote_and_empty(hctx):
    a, b, by_type, _ = make_twins(hctx, seed=51, labels=False)
    multi = sorted((p, v) for p, v in ids_of(by_type)[0].items() if len(v) >= 2)
    assert len(multi) > 40
    demote = [(0, s, d, i) for (s, d), v in multi[0::4] for i in v[1:]]    # all but the smallest id
    empty = [(0, s, d, i) for (s, d), v in multi[1::4] for i in v]         # every id
    shrink = [(0, s, d, v[-1]) for (s, d), v in multi[2::4] if len(v) >= 3]   # one of three or more
    batch = demote + empty + shrink
    want = delete_edges(by_type, batch)
    edge_by_edge(a, batch)
    rels, st = bulk(b, batch[::-1], stats=True)
    assert sorted(rels) == sorted(want["list"]) and st["edges_removed"] == len(batch)
    assert st["pairs_demoted"] == len(multi[0::4]) and st["pairs_emptied"] == len(multi[1::4])
    for (s, d), v in multi[2::4]:
        assert b.tensor_get(0, s, d) == (v[:-1] if len(v) >= 3 else v)
    for (s, d), v in multi[0::4]:
        assert b.tensor_get(0, s, d) == [v[0]]
    for (s, d), v in multi[1::4]:
        assert b.tensor_get(0, s, d) == []
    assert_twins(a, b, [p for p, _ in multi][:100])
    assert_state(b, want)


def test_a_pair_both_types_share_loses_one_type_only(hctx):
    a, b, by_type, _ = make_twins(hctx, seed=61, labels=False)
    r_ids, s_ids = ids_of(by_type)
    shared = sorted(set(r_ids) & set(s_ids))[:30]
    assert len(shared) == 30
    batch = [(0, s, d, i) for s, d in shared for i in r_ids[(s, d)]]       # every R edge of the pair; S keeps its own
    only_r = sorted(set(r_ids) - set(s_ids))[:10]
    batch += [(0, s, d, i) for s, d in only_r for i in r_ids[(s, d)]]      # ... and pairs nothing else connects
    want = delete_edges(by_type, batch)
    edge_by_edge(a, batch)
    rels, st = bulk(b, batch, stats=True)
    assert rels == want["list"] and st["pairs_emptied"] == 40 and st["adjacency_entries"] == 10
    adj = eff_adjacency(b)
    assert all(p in adj for p in shared) and not any(p in adj for p in only_r)
    assert_twins(a, b, shared + only_r)
    assert_state(b, want)


def test_unfolded_deltas_before_the_call(hctx):
    """Edges created and deleted edge by edge, with no commit, leave dp and dm populated: the call folds them first."""
    a, b, by_type, _ = make_twins(hctx, seed=31, labels=False)
    extra = [(3, 7, 9000), (3, 7, 9004), (250, 251, 9001), (8, 8, 9002)]
    gone = by_type[0][:25]
    for g in (a, b):
        for s, d, i in extra:
            g.create_edge(0, s, d, i)
        for s, d, i in gone:
            g.delete_edge(0, s, d, i)
    st = b.tensor_state(0)
    assert st["dp"] > 0 and st["dm"] > 0
    by_type[0] = by_type[0][25:] + extra
    batch = [(0, s, d, i) for s, d, i in by_type[0][5:60]] + [(0, 3, 7, 9004), (0, 8, 8, 9002)] + [(0,) + gone[0]]
    want = delete_edges(by_type, batch)
    edge_by_edge(a, batch)
    assert bulk(b, batch) == want["list"]
    assert_twins(a, b, probes_of(by_type, batch))
    assert_state(b, want)
    assert 9000 in b.tensor_get(0, 3, 7) and 9001 in b.tensor_get(0, 250, 251)     # the folded delta is still there


def test_an_indexed_edge_leaves_its_vector_index(hctx):
    g = host.Graph(hctx, 40)
    knows = g.add_type("Knows")
    g.vector_index_create(True, knows, "emb", 2, None)
    s, d = np.arange(30, dtype=np.uint64), (np.arange(30, dtype=np.uint64) + 1) % 30
    g.bulk_insert_edges(knows, s, d, np.arange(100, 130, dtype=np.uint64))
    for v in range(30):
        g.vector_set_edge(knows, "emb", v, (v + 1) % 30, 100 + v, [v, 1])
    rels = g.delete_edges_bulk(knows, [4, 5, 19], [5, 6, 20], [104, 105, 119])
    assert rels == [(104, 4, 5), (105, 5, 6), (119, 19, 20)]
    edges, _, _, _ = g.vector_query_edges("Knows", "emb", 100, [0, 0])
    assert sorted(edges.tolist()) == [100 + v for v in range(30) if v not in (4, 5, 19)]


def test_the_explicit_delete_after_a_bulk_node_delete_finds_nothing(hctx):
    """delete_nodes_bulk(D, skip_ids=X) removes X's edges without listing them; the delete_edges_bulk(X) that follows, as in
    Pending::commit, hits nothing and leaves the state as it is."""
    a, b, by_type, _ = make_twins(hctx, seed=21, labels=False)
    D = pick_nodes(by_type, k=12, seed=4)
    Ds = set(D)
    incident = [(t, s, d, i) for t, _ in TYPES for s, d, i in by_type[t] if s in Ds or d in Ds]
    X = incident[::3]
    listed = b.delete_nodes_bulk(D, skip_ids=[x[3] for x in X])
    assert len(listed) == len(incident) - len(X)
    state = [b.tensor_state(t) for t, _ in TYPES]
    edges = [sorted(b.tensor_iter_edges(t)) for t, _ in TYPES]
    adj = eff_adjacency(b)
    rels, st = bulk(b, X, stats=True)
    assert rels == [] and st["edges_named"] == len(X)
    assert st["edges_removed"] == st["pairs_emptied"] == st["pairs_demoted"] == st["adjacency_entries"] == 0
    assert [b.tensor_state(t) for t, _ in TYPES] == state and eff_adjacency(b) == adj
    assert [sorted(b.tensor_iter_edges(t)) for t, _ in TYPES] == edges


def test_an_unknown_type_and_a_node_past_the_capacity_throw_with_the_graph_unchanged(hctx):
    a, b, by_type, _ = make_twins(hctx, seed=41, labels=False)
    state = [b.tensor_state(t) for t, _ in TYPES]
    adj = eff_adjacency(b)
    s, d, i = by_type[0][0]
    for bad in ([(0, s, d, i), (2, s, d, i)], [(0, s, d, i), (1, N, 0, 5)], [(1, 0, N, 5), (0, s, d, i)]):
        with pytest.raises(host.HostError) as e:
            bulk(b, bad)
        assert e.value.code == _ffi.FGPU_INVALID
        assert [b.tensor_state(t) for t, _ in TYPES] == state and eff_adjacency(b) == adj
        assert i in b.tensor_get(0, s, d)                                  # the good edge of the batch is still there
    rels, st = b.delete_edges_bulk([], [], [], [], stats=True)            # an empty batch does nothing
    assert rels == [] and st["edges_named"] == 0 and st["edges_removed"] == 0
    assert [b.tensor_state(t) for t, _ in TYPES] == state
    assert_twins(a, b, [(s, d)])                                           # (twin a was never touched)
