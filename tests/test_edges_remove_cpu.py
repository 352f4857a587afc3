"""tests/edges_remove_check.py pinned on expectations written out by hand from tensor.rs:497-629 — the checker of
fgpu_edges_remove and Graph::delete_edges_bulk must not be whatever the device code happens to compute.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edges_remove_check import MULTI, delete_edges, remove_edges  # noqa: E402

# a 6 x 6 tensor: (0, 1) and (5, 5) single, (2, 3) with three edges, (4, 0) with two, (1, 1) a self-loop pair with two
PAIRS = {(0, 1): 10, (2, 3): MULTI, (4, 0): MULTI, (5, 5): 77, (1, 1): MULTI, (3, 2): 31}
ROWS = {(2, 3): [20, 21, 25], (4, 0): [40, 44], (1, 1): [11, 12]}
N_ROW_IDS = 7


def run(triples, pairs=PAIRS, rows=ROWS):
    return remove_edges(pairs, rows, triples)


def test_an_inline_hit():
    kept, hit, taken, emptied, st = run([(0, 1, 10)])
    assert (0, 1) not in kept and len(kept) == 5 and kept[(2, 3)] == MULTI
    assert hit == [1] and taken == [0] * N_ROW_IDS and emptied == [(0, 1)]
    assert st == [1, 1, 0, 0, 5, 5, 0, 0]


def test_an_unknown_id_on_a_single_pair():
    """:583-584 — the slow path skips it; the no-multi fast path (:467-495) would drop the pair, the contract does not."""
    kept, hit, taken, emptied, st = run([(0, 1, 99)])
    assert kept == PAIRS and hit == [0] and emptied == [] and st == [0, 0, 0, 0, 6, 6, 0, 1]
    kept, hit, _, emptied, st = remove_edges({(0, 1): 10}, {}, [(0, 1, 99)])   # ... also without any multi-edge pair
    assert kept == {(0, 1): 10} and hit == [0] and emptied == [] and st == [0, 0, 0, 0, 1, 1, 0, 1]


def test_an_absent_pair():
    kept, hit, taken, emptied, st = run([(0, 2, 10), (3, 3, 1)])
    assert kept == PAIRS and hit == [0, 0] and taken == [0] * N_ROW_IDS and emptied == [] and st == [0, 0, 0, 0, 6, 6, 2, 0]


def test_an_id_of_another_pair():
    """21 lives on (2, 3): naming it on (4, 0) (multi) and on (5, 5) (single) removes nothing anywhere."""
    kept, hit, taken, emptied, st = run([(4, 0, 21), (5, 5, 21)])
    assert kept == PAIRS and hit == [0, 0] and taken == [0] * N_ROW_IDS and emptied == [] and st == [0, 0, 0, 0, 6, 6, 0, 2]


def test_a_multi_pair_going_from_three_to_two():
    kept, hit, taken, emptied, st = run([(2, 3, 21)])
    assert kept == PAIRS and kept[(2, 3)] == MULTI                      # still MULTI: two ids are left
    assert hit == [1] and taken == [0, 0, 0, 1, 0, 0, 0]                # rows in (src, dst) order: (1,1) (2,3) (4,0)
    assert emptied == [] and st == [1, 0, 0, 0, 6, 6, 0, 0]


def test_a_multi_pair_going_from_two_to_one_demotes():
    kept, hit, taken, emptied, st = run([(4, 0, 40)])
    assert kept == {**PAIRS, (4, 0): 44}                                # the survivor is inline
    assert hit == [1] and taken == [0, 0, 0, 0, 0, 1, 0] and emptied == [] and st == [1, 0, 0, 1, 6, 6, 0, 0]
    kept, _, taken, _, st = run([(2, 3, 25), (2, 3, 20)])               # 3 -> 1 in one batch: the middle id survives
    assert kept[(2, 3)] == 21 and taken == [0, 0, 1, 0, 1, 0, 0] and st == [2, 0, 0, 1, 6, 6, 0, 0]


def test_a_multi_pair_whose_ids_all_go_in_one_batch():
    """:563-575 — the pair demotes after the second removal, and the third triple names the inline survivor: emptied."""
    kept, hit, taken, emptied, st = run([(2, 3, 20), (2, 3, 25), (2, 3, 21), (1, 1, 12), (1, 1, 11)])
    assert (2, 3) not in kept and (1, 1) not in kept and len(kept) == 4
    assert hit == [1] * 5 and taken == [1, 1, 1, 1, 1, 0, 0] and emptied == [(1, 1), (2, 3)]
    assert st == [5, 2, 2, 0, 4, 4, 0, 0]


def test_a_duplicated_triple():
    """The second copy finds the id gone in the reference (:546-550, :583-584) and changes nothing; both hit flags are 1."""
    kept, hit, taken, emptied, st = run([(0, 1, 10), (2, 3, 20), (0, 1, 10), (2, 3, 20)])
    assert (0, 1) not in kept and kept[(2, 3)] == MULTI and hit == [1, 1, 1, 1]
    assert taken == [0, 0, 1, 0, 0, 0, 0] and emptied == [(0, 1)] and st == [4, 1, 0, 0, 5, 5, 0, 0]


def test_the_full_matrix_contract_on_6_by_6():
    triples = [(5, 5, 77), (2, 3, 25), (4, 0, 44), (4, 0, 40), (1, 1, 11), (3, 2, 30), (0, 0, 5), (2, 3, 40), (5, 5, 77)]
    kept, hit, taken, emptied, st = run(triples)
    assert kept == {(0, 1): 10, (2, 3): MULTI, (1, 1): 12, (3, 2): 31}
    assert hit == [1, 1, 1, 1, 1, 0, 0, 0, 1]
    assert taken == [1, 0, 0, 0, 1, 1, 1]
    assert emptied == [(4, 0), (5, 5)]
    #            hits emptied multi demoted kept kept absent unknown
    assert st == [6, 2, 1, 1, 4, 4, 1, 2]


def test_a_supplied_row_of_a_pair_that_is_not_multi_is_ignored_and_a_missing_row_is_an_error():
    kept, hit, taken, emptied, st = remove_edges({(0, 1): 10}, {(0, 1): [10, 11], (3, 3): [1, 2]}, [(0, 1, 10)])
    assert kept == {} and hit == [1] and taken == [0, 0, 0, 0] and emptied == [(0, 1)] and st == [1, 1, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        remove_edges({(2, 3): MULTI}, {}, [(2, 3, 20)])


def test_the_graph_level_list_and_adjacency():
    by_type = [[(0, 1, 10), (2, 3, 20), (2, 3, 21)], [(0, 1, 50), (4, 4, 51)]]
    batch = [(1, 4, 4, 51), (0, 2, 3, 21), (0, 0, 1, 10), (0, 2, 3, 21), (1, 0, 1, 10), (0, 9, 9, 1)]
    want = delete_edges(by_type, batch)
    assert want["list"] == [(21, 2, 3), (10, 0, 1), (51, 4, 4)]         # type 0 in input order, then type 1
    assert want["edges"] == [[(2, 3, 20)], [(0, 1, 50)]]
    assert want["adjacency"] == {(2, 3), (0, 1)}                        # (0, 1) lost type 0 only: type 1 still connects it
