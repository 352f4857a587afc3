"""GPU: db.idx.vector.queryNodes / queryRelationships and vec.*Distance through the host layer (fh_graph_vector_*,
fh_vector_query_*, fh_vec_distance) on the data of the reference's tests/flow/test_vecsim.py, restated: 1001 Person nodes with
embeddings = (i, i) under euclidean and embedding2 = (i, sin(i + 1)) under cosine, and 1001 self-loop Points relationships
with embeddings = (-id, -id)."""
import math
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host
from falkordb_amd.host import HostError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vec_check as vc  # noqa: E402

pytestmark = pytest.mark.gpu
N = 1001


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vecsim(hctx):
    """(graph, Person label id, Points type id, embeddings, embedding2, edge embeddings)"""
    g = host.Graph(hctx, N)
    person, points = g.add_label("Person"), g.add_type("Points")
    i = np.arange(N, dtype=np.float64)
    e1 = np.stack([i, i], axis=1).astype(np.float32)
    e2 = np.stack([i, np.sin(i + 1)], axis=1).astype(np.float32)
    ee = -e1
    ids = np.arange(N, dtype=np.uint64)
    g.create_edges(points, ids, ids, ids)
    g.vector_index_create(False, person, "embeddings", 2, "euclidean")
    g.vector_index_create(False, person, "embedding2", 2, "cosine")
    g.vector_index_create(True, points, "embeddings", 2, None)   # NULL = euclidean
    for n in range(N):
        g.label_node(n, person)
        g.vector_set_node(person, "embeddings", n, e1[n])
        g.vector_set_node(person, "embedding2", n, e2[n])
        g.vector_set_edge(points, "embeddings", n, n, n, ee[n])
    return g, person, points, e1, e2, ee


def test_query_nodes_k3(vecsim):   # test02
    g, _, _, e1, _, _ = vecsim
    nodes, scores = g.vector_query_nodes("Person", "embeddings", 3, [50, 50])
    assert len(nodes) == 3 and len(scores) == 3
    for n in nodes:
        assert abs(e1[n][0] - 50) < 3 and abs(e1[n][1] - 50) < 3
    assert nodes.tolist() == [50, 49, 51] and scores.tolist() == [0.0, math.sqrt(2.0), math.sqrt(2.0)]


def test_query_relationships_k3(vecsim):   # test03
    g, _, _, _, _, ee = vecsim
    rels, scores, srcs, dsts = g.vector_query_edges("Points", "embeddings", 3, [-50, -50])
    assert len(rels) == 3
    for r, s, d in zip(rels, srcs, dsts):
        assert abs(ee[r][0] + 50) < 3 and abs(ee[r][1] + 50) < 3
        assert s == r and d == r
    assert rels.tolist() == [50, 49, 51]


def test_scores_ascend_and_equal_vec_distance(vecsim):   # test04
    g, _, _, e1, e2, ee = vecsim
    q = np.array([50, 50], dtype=np.float32)
    for attr, store, metric in (("embeddings", e1, "euclidean"), ("embedding2", e2, "cosine")):
        nodes, scores = g.vector_query_nodes("Person", attr, 100, q)
        assert len(nodes) == 100 and np.all(np.diff(scores) >= 0)
        for n, s in zip(nodes, scores):
            assert round(s, 3) == round(host.vec_distance(metric, store[n], q), 3)
        want = vc.dist(metric, q, store)
        assert np.all(np.abs(scores - want[nodes.astype(np.int64)]) <= 1e-12 * np.maximum(1.0, np.abs(scores)))
    rels, scores, _, _ = g.vector_query_edges("Points", "embeddings", 100, -q)
    assert len(rels) == 100 and np.all(np.diff(scores) >= 0)
    for r, s in zip(rels, scores):
        assert round(s, 3) == round(host.Graph.vec_distance("euclidean", ee[r], -q), 3)


def test_k_larger_than_the_index(vecsim):   # test05
    g = vecsim[0]
    nodes, scores = g.vector_query_nodes("Person", "embeddings", 1000000, [50, 50])
    assert len(nodes) == N and sorted(nodes.tolist()) == list(range(N)) and np.all(np.diff(scores) >= 0)
    rels, _, srcs, dsts = g.vector_query_edges("Points", "embeddings", 1000000, [50, 50])
    assert len(rels) == N and np.array_equal(rels, srcs) and np.array_equal(rels, dsts)


def message_of(call):
    with pytest.raises(HostError) as e:
        call()
    return str(e.value).split(": ", 1)[1]


def test_error_texts(vecsim):   # test07 and the argument checks of the two procedures
    g, person, points = vecsim[:3]
    assert message_of(lambda: g.vector_query_nodes("Person", "embeddings", 3, [1, 2, 3])) == \
        "Vector dimension mismatch, expected 2 but got 3"
    assert message_of(lambda: g.vector_query_edges("Points", "embeddings", 3, [1])) == \
        "Vector dimension mismatch, expected 2 but got 1"
    assert message_of(lambda: host.vec_distance("euclidean", [1, 2], [1, 2, 3])) == \
        "Vector dimension mismatch, expected 2 but got 3"
    assert "Vector dimension mismatch" in message_of(lambda: host.vec_distance("cosine", [1, 2, 3], [1]))
    for k in (0, -1):
        assert message_of(lambda: g.vector_query_nodes("Person", "embeddings", k, [1, 2])) == \
            "Invalid arguments for procedure 'db.idx.vector.queryNodes'"
        assert message_of(lambda: g.vector_query_edges("Points", "embeddings", k, [1, 2])) == \
            "Invalid arguments for procedure 'db.idx.vector.queryRelationships'"
    assert message_of(lambda: g.vector_index_create(False, person, "other", 2, "manhattan")) == \
        "Unknown similarity function 'manhattan', expected 'euclidean', 'ip', or 'cosine'"
    assert message_of(lambda: g.vector_set_node(person, "embeddings", 5, [1, 2, 3])) == \
        "Vector dimension mismatch, expected 2 but got 3"
    with pytest.raises(HostError):
        g.vector_set_node(person, "nothing", 5, [1, 2])
    with pytest.raises(HostError):
        g.vector_set_node(person, "embeddings", 5, [1, float("nan")])
    with pytest.raises(HostError):
        g.vector_index_create(False, person, "embeddings", 2, "euclidean")   # indexed already
    # none of it changed anything
    assert g.vector_query_nodes("Person", "embeddings", 1, [5, 5])[0].tolist() == [5]


def test_vec_distance():
    assert round(host.vec_distance("euclidean", [1, 2], [2, 3]), 3) == 1.414   # test01
    assert round(host.vec_distance("cosine", [1, 2], [2, 3]), 3) == 0.008
    assert host.vec_distance("cosine", [0, 0], [2, 3]) == 1.0
    assert host.vec_distance("ip", [1, 2], [2, 3]) == -8.0
    rng = np.random.default_rng(9)
    a, b = rng.uniform(-1, 1, (2, 130)).astype(np.float32)
    for metric in vc.METRICS:
        want = vc.dist(metric, a, b)[0]
        assert abs(host.vec_distance(metric, a, b) - want) <= 1e-12 * max(1.0, abs(want))


def test_missing_index_gives_no_rows(vecsim):
    g = vecsim[0]
    for label, attr in (("Person", "nothing"), ("Nobody", "embeddings")):
        nodes, scores = g.vector_query_nodes(label, attr, 3, [1, 2])
        assert len(nodes) == 0 and len(scores) == 0
    assert all(len(a) == 0 for a in g.vector_query_edges("Points", "nothing", 3, [1, 2]))
    assert all(len(a) == 0 for a in g.vector_query_edges("Nothing", "embeddings", 3, [1, 2]))
    off, nodes, _ = g.vector_query_nodes_batch("Person", "nothing", 3, np.zeros((4, 2), dtype=np.float32))
    assert off.tolist() == [0] * 5 and len(nodes) == 0


def test_batch_of_1024_equals_single_calls(vecsim):
    g, _, _, e1, _, _ = vecsim
    rng = np.random.default_rng(4)
    queries = rng.uniform(0, 1000, (1024, 2)).astype(np.float32)
    off, nodes, scores = g.vector_query_nodes_batch("Person", "embeddings", 5, queries)
    assert off.tolist() == list(range(0, 5 * 1024 + 1, 5))
    for r in range(1024):
        n1, s1 = g.vector_query_nodes("Person", "embeddings", 5, queries[r])
        assert np.array_equal(n1, nodes[off[r]:off[r + 1]]), f"query {r}"
        assert np.array_equal(s1.view(np.uint64), scores[off[r]:off[r + 1]].view(np.uint64)), f"query {r}"
    # and they are the nearest: against the checker, through the band rule of the float tests
    for r in range(0, 1024, 64):
        keys = vc.keys64("euclidean", queries[r], e1)
        assert vc.band_ok(nodes[off[r]:off[r + 1]], 5, keys, vc.margin("euclidean", queries[r], e1))


def test_deleted_entities_leave_their_indexes(hctx):   # test09
    g = host.Graph(hctx, 16)
    person, points = g.add_label("Person"), g.add_type("Points")
    g.vector_index_create(False, person, "embeddings", 2, "euclidean")
    g.vector_index_create(False, person, "embedding2", 2, "cosine")
    g.vector_index_create(True, points, "embeddings", 2, "euclidean")
    g.label_node(3, person)
    g.vector_set_node(person, "embeddings", 3, [2, 2])
    g.vector_set_node(person, "embedding2", 3, [2, 2])
    assert g.vector_query_nodes("Person", "embeddings", 1, [2, 2])[0].tolist() == [3]
    g.delete_node(3)
    for attr in ("embeddings", "embedding2"):
        assert len(g.vector_query_nodes("Person", attr, 1, [2, 2])[0]) == 0
    g.label_node(4, person)
    g.vector_set_node(person, "embeddings", 4, [2, 2])
    assert g.vector_query_nodes("Person", "embeddings", 1, [2, 2])[0].tolist() == [4]
    # relationships
    g.create_edge(points, 1, 2, 7)
    g.create_edge(points, 2, 5, 8)
    g.vector_set_edge(points, "embeddings", 1, 2, 7, [1, 1])
    g.vector_set_edge(points, "embeddings", 2, 5, 8, [9, 9])
    rels, _, srcs, dsts = g.vector_query_edges("Points", "embeddings", 2, [1, 1])
    assert (rels.tolist(), srcs.tolist(), dsts.tolist()) == ([7, 8], [1, 2], [2, 5])
    with pytest.raises(HostError):
        g.delete_edge(99, 1, 2, 7)   # no such type: the delete fails and the relationship keeps its vector
    assert g.vector_query_edges("Points", "embeddings", 2, [1, 1])[0].tolist() == [7, 8]
    g.delete_edge(points, 1, 2, 7)
    rels, _, srcs, dsts = g.vector_query_edges("Points", "embeddings", 2, [1, 1])
    assert (rels.tolist(), srcs.tolist(), dsts.tolist()) == ([8], [2], [5])
    # unset and drop
    assert g.vector_unset_edge(points, "embeddings", 8) and not g.vector_unset_edge(points, "embeddings", 8)
    assert g.vector_unset_node(person, "embeddings", 4) and not g.vector_unset_node(person, "embeddings", 4)
    assert g.vector_index_drop(False, person, "embeddings") and not g.vector_index_drop(False, person, "embeddings")
    assert len(g.vector_query_nodes("Person", "embeddings", 1, [2, 2])[0]) == 0


def test_delete_node_without_an_index_is_untouched(hctx):
    g = host.Graph(hctx, 8)
    t = g.add_type("T")
    g.create_edge(t, 0, 1, 0)
    g.create_edge(t, 2, 3, 1)
    g.delete_node(5)
    g.delete_edge(t, 2, 3, 1)
    nodes, comp = g.algo_wcc()
    assert nodes.tolist() == [0, 1, 2, 3, 4, 6, 7] and comp.tolist() == [0, 0, 2, 3, 4, 6, 7]
