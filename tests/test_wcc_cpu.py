"""CPU: the WCC checker of tests/wcc_check.py (min-label propagation + pointer jumping) against a plain union-find."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wcc_check import components, csr_of, union_find_labels, wcc_labels  # noqa: E402


def _check(n, rows, cols, active=None):
    rp, ci = csr_of(n, rows, cols)
    got = wcc_labels(n, rp, ci, active)
    want = union_find_labels(n, rows, cols, active)
    assert np.array_equal(got, want)
    return got


def test_hand_graphs():
    assert len(_check(0, [], [])) == 0
    assert _check(1, [], []).tolist() == [0]
    assert _check(3, [0, 0, 2, 2], [0, 0, 2, 2]).tolist() == [0, 1, 2]          # self-loops and duplicates
    assert _check(6, [5, 4], [4, 3]).tolist() == [0, 1, 2, 3, 3, 3]             # the minimum at the far end of a path
    assert _check(5, [0, 0, 0, 0], [1, 2, 3, 4]).tolist() == [0] * 5            # a star
    path = _check(50, np.arange(49), np.arange(1, 50))
    assert (path == 0).all()
    rev = _check(50, np.arange(1, 50)[::-1], np.arange(49)[::-1])
    assert (rev == 0).all()


def test_active_mask_cuts_paths():
    act = np.ones(5, dtype=bool)
    act[2] = False
    got = _check(5, [0, 1, 2, 3], [1, 2, 3, 4], act)
    assert got.tolist() == [0, 0, -1, 3, 3]
    assert components(got) == 2


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs_match_union_find(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 300))
    m = int(rng.integers(0, 2 * n))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    _check(n, rows, cols)
    _check(n, rows, cols, rng.random(n) < 0.7)
