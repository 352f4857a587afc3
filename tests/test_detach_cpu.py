"""CPU: tests/detach_check.py on hand-derived cases of the reference's cascade delete.  Every expectation below is written out
from graph.rs:2386-2494 (delete_implicit_edges) and graph.rs:1753-1768 (the label rows of delete_nodes) by hand, not computed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detach_check import MULTI, delete_nodes, detach_matrix, implicit_edges  # noqa: E402


def test_an_out_edge_and_an_in_edge():
    """Node 5 deleted: its outgoing walk (:2407-2413) meets 5->7, its incoming walk (:2417-2426) 2->5."""
    edges = [(2, 5, 10), (5, 7, 11), (2, 7, 12)]
    assert implicit_edges(edges, [5]) == [(11, 5, 7), (10, 2, 5)]
    r = delete_nodes([edges], [5])
    assert r["list"] == [(11, 5, 7), (10, 2, 5)] and r["edges"] == [[(2, 7, 12)]] and r["adjacency"] == {(2, 7)}


def test_out_edges_by_dst_then_in_edges_by_src_per_node_ascending():
    """Nodes 3 and 1 deleted, named out of order: node 1 first (:2405), each node's out edges before its in edges."""
    edges = [(3, 9, 1), (3, 4, 2), (8, 3, 3), (6, 3, 4), (1, 9, 5), (7, 1, 6)]
    assert implicit_edges(edges, [3, 1]) == [(5, 1, 9), (6, 7, 1), (2, 3, 4), (1, 3, 9), (4, 6, 3), (3, 8, 3)]


def test_both_endpoints_deleted_is_listed_once_from_the_source():
    """4->6 with 4 and 6 deleted: found in 4's outgoing walk; 6's incoming walk skips it because 4 is deleted (:2421)."""
    edges = [(4, 6, 20), (6, 4, 21), (4, 9, 22)]
    r = delete_nodes([edges], [6, 4])
    assert r["list"] == [(20, 4, 6), (22, 4, 9), (21, 6, 4)]
    assert r["edges"] == [[]] and r["adjacency"] == set()
    assert r["adjacency_reference"] == {(4, 6), (6, 4)}                  # :2381-2383: left behind as unreachable


def test_a_self_loop_is_listed_once():
    """3->3 with 3 deleted: the outgoing walk lists it, the incoming walk skips src == node (:2420)."""
    assert implicit_edges([(3, 3, 7), (1, 3, 8)], [3]) == [(7, 3, 3), (8, 1, 3)]
    assert implicit_edges([(3, 3, 7), (1, 3, 8)], [1]) == [(8, 1, 3)]     # a surviving node's loop stays


def test_a_multi_edge_pair_lists_its_ids_ascending():
    edges = [(2, 5, 31), (2, 5, 30), (2, 5, 35), (5, 2, 33), (5, 2, 32)]
    assert implicit_edges(edges, [5]) == [(32, 5, 2), (33, 5, 2), (30, 2, 5), (31, 2, 5), (35, 2, 5)]


def test_a_skipped_id_is_not_listed_and_does_not_survive():
    """explicit_rels (:2410, :2422): the id is left out; once the explicit delete has run too the edge is gone either way."""
    edges = [(2, 5, 10), (5, 7, 11), (5, 7, 12), (1, 2, 13)]
    r = delete_nodes([edges], [5], skip_ids=[11, 10])
    assert r["list"] == [(12, 5, 7)] and r["edges"] == [[(1, 2, 13)]]


def test_two_types_sharing_a_pair_come_type_by_type():
    """:2401: the outer loop is over the types; the shared pair 1->2 is listed under each."""
    r = delete_nodes([[(1, 2, 100), (3, 1, 101)], [(1, 2, 200), (2, 3, 201)]], [1])
    assert r["list"] == [(100, 1, 2), (101, 3, 1), (200, 1, 2)]
    assert r["edges"] == [[], [(2, 3, 201)]] and r["adjacency"] == {(2, 3)}


def test_a_node_without_edges_and_the_label_rows():
    """:1753-1768: the deleted nodes' label rows go; a node with no edge lists nothing."""
    r = delete_nodes([[(1, 2, 5)]], [9, 4], labels=[(9, 0), (9, 3), (1, 0), (4, 1), (2, 1)])
    assert r["list"] == [] and r["edges"] == [[(1, 2, 5)]] and r["labels"] == [(1, 0), (2, 1)]
    assert delete_nodes([[]], [], labels=[(1, 0)])["labels"] == [(1, 0)]


def test_the_matrix_contract_by_hand():
    """fgpu_nodes_detach's own statement on one 6 x 6 matrix, D = {1, 4}."""
    e = {(0, 1): 7, (1, 1): 8, (1, 3): MULTI, (2, 4): 9, (4, 1): 10, (5, 0): 11, (3, 1): MULTI}
    kept, out, inn, st = detach_matrix(e, [4, 1, 1], 3)
    assert kept == {(5, 0): 11}
    assert out == [(1, 1, 8), (1, 3, MULTI), (4, 1, 10)]                  # ascending (src, dst); the loop and 4->1 here only
    assert inn == [(0, 1, 7), (3, 1, MULTI), (2, 4, 9)]                   # ascending (dst, src), sources outside D
    assert st == [2, 3, 3, 2, 1, 1]
    kept, out, inn, st = detach_matrix(e, [1, 4], 1)                      # rows only: the label matrix' form
    assert sorted(kept) == [(0, 1), (2, 4), (3, 1), (5, 0)] and len(out) == 3 and inn == [] and st == [2, 3, 0, 1, 4, 4]
    kept, out, inn, st = detach_matrix(e, [1, 4], 2)                      # columns only: everything removed is an in entry
    assert sorted(kept) == [(1, 3), (5, 0)] and out == [] and inn == [(0, 1, 7), (1, 1, 8), (3, 1, MULTI), (4, 1, 10), (2, 4, 9)]
