"""CPU: the CDLP checker of tests/cdlp_check.py (lexsort + run-length encoding) against plain dict counting, and the
hand-worked cases that pin the rules of include/fgpu.h (fgpu_cdlp)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdlp_check import cdlp_labels, cdlp_stats, csr_of, dict_labels  # noqa: E402


def sym(rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


def run(n, rows, cols, itermax, active=None):
    rp, ci = csr_of(n, rows, cols)
    return cdlp_labels(n, rp, ci, itermax, active)


@pytest.mark.parametrize("seed", range(8))
def test_checker_matches_dict_counting(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 60))
    m = int(rng.integers(0, 4 * n))
    rows, cols = sym(rng.integers(0, n, m), rng.integers(0, n, m))          # duplicates and self-loops included
    active = None if seed % 2 == 0 else rng.random(n) < 0.7
    for itermax in (0, 1, 2, 3, 10):
        got = run(n, rows, cols, itermax, active)
        want = dict_labels(n, rows, cols, itermax, active)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


def test_a_tie_goes_to_the_smaller_label():
    # vertex 4 sees 1, 2 and 3 once each; vertex 5 sees 2 and 3
    rows, cols = sym([4, 4, 4, 5, 5], [3, 1, 2, 3, 2])
    lab, _, _ = run(6, rows, cols, 1)
    assert lab[4] == 1 and lab[5] == 2
    # two votes for 7 beat one vote for 0: frequency first, the label only breaks ties
    # (vertex 6 takes label 7 in iteration 1, vertex 8 counts {0: 1, 7: 2} in iteration 2)
    rows, cols = [6, 8, 8, 8, 7], [7, 0, 7, 6, 7]
    got, _, _ = run(9, rows, cols, 2)
    assert got[6] == 7 and got[8] == 7


def test_a_two_path_oscillates_with_period_two():
    rows, cols = sym([0], [1])
    assert run(2, rows, cols, 1)[0].tolist() == [1, 0]
    assert run(2, rows, cols, 2)[0].tolist() == [0, 1]
    a, b = run(2, rows, cols, 3), run(2, rows, cols, 4)
    assert a[0].tolist() == [1, 0] and b[0].tolist() == [0, 1]
    assert a[1:] == (3, 2) and b[1:] == (4, 2)                               # never converged: itermax ended both


def test_a_self_loop_votes():
    # 2 - 3: vertex 2 takes 3.  With a loop on 2 it counts {2: 1, 3: 1} and the tie keeps 2
    rows, cols = sym([2], [3])
    assert run(4, rows, cols, 1)[0].tolist() == [0, 1, 3, 2]
    rows, cols = np.append(rows, 2), np.append(cols, 2)
    assert run(4, rows, cols, 1)[0].tolist() == [0, 1, 2, 2]
    # a duplicate pair is one entry and one vote: two copies of the loop do not outvote the neighbour ... the tie stays
    rows, cols = np.append(rows, 2), np.append(cols, 2)
    assert run(4, rows, cols, 1)[0].tolist() == [0, 1, 2, 2]
    # a loop alone keeps the label and converges at once
    lab, it, ch = run(3, [1], [1], 10)
    assert lab.tolist() == [0, 1, 2] and (it, ch) == (1, 0)


def test_an_isolated_vertex_keeps_its_id_and_itermax_zero_is_the_identity():
    rows, cols = sym([0, 1], [1, 2])
    lab, it, ch = run(5, rows, cols, 10)
    assert lab[3] == 3 and lab[4] == 4
    lab, it, ch = run(5, rows, cols, 0)
    assert lab.tolist() == [0, 1, 2, 3, 4] and (it, ch) == (0, 0)
    act = np.array([True, True, False, True, False])
    lab, st = cdlp_stats(5, *csr_of(5, rows, cols), 0, act)
    assert lab.tolist() == [0, 1, -1, 3, -1] and st == [0, 0, 0, 3]


def test_a_triangle_converges_early_and_inactive_columns_do_not_vote():
    rows, cols = sym([0, 1, 2], [1, 2, 0])
    lab, it, ch = run(3, rows, cols, 10)
    # t1: 0 <- min(1, 2) = 1, 1 <- 0, 2 <- 0; t2: 0 <- {0: 2}, 1 and 2 <- {1: 1, 0: 1} -> 0; t3 changes nothing
    assert lab.tolist() == [0, 0, 0] and (it, ch) == (3, 0)
    act = np.array([True, True, False])
    lab, st = cdlp_stats(3, *csr_of(3, rows, cols), 3, act)
    # the 2-path 0 - 1 oscillates, 2 is out; the two active rows store 4 entries
    assert lab.tolist() == [1, 0, -1] and st == [3, 2, 3 * 4, 2]
