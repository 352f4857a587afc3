"""CPU: the max-flow checker and value solver of tests/maxflow_check.py against hand cases and deliberately broken flows, and
the binding of fgpu_maxflow against its declaration."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maxflow_check import certify, dinic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the textbook network: 0 = s, 5 = t, maximum flow 23
ROWS = np.array([0, 0, 1, 2, 1, 3, 2, 4, 3, 4])
COLS = np.array([1, 2, 2, 1, 3, 2, 4, 3, 5, 5])
CAPS = np.array([16, 13, 10, 4, 12, 9, 14, 7, 20, 4], dtype=np.float64)
# one of its maximum flows, sorted by (row, col)
FLOW = [(0, 1, 12.0), (0, 2, 11.0), (1, 3, 12.0), (2, 4, 11.0), (3, 5, 19.0), (4, 3, 7.0), (4, 5, 4.0)]


def run(flow, value=23.0, **kw):
    r, c, f = (np.array(x) for x in zip(*flow))
    return certify(6, ROWS, COLS, CAPS, 0, 5, value, r, c, f, **kw)


def test_checker_accepts_a_known_maximum_flow():
    run(FLOW)
    certify(3, [0], [1], [5.0], 0, 2, 0.0, [], [], [])   # no path: the empty flow is maximal


def test_checker_rejects_a_preflow():
    # 13 leave src towards 2, only 11 go on: vertex 2 keeps an excess of 2
    bad = [(0, 1, 12.0), (0, 2, 13.0), (1, 3, 12.0), (2, 4, 11.0), (3, 5, 19.0), (4, 3, 7.0), (4, 5, 4.0)]
    with pytest.raises(AssertionError, match="preflow"):
        run(bad)


def test_checker_rejects_an_over_capacity_entry():
    bad = [(0, 1, 12.0), (0, 2, 11.0), (1, 3, 12.0), (2, 4, 11.0), (3, 5, 18.0), (4, 3, 7.0), (4, 5, 5.0)]
    with pytest.raises(AssertionError, match="capacity"):
        run(bad)
    with pytest.raises(AssertionError, match="not a live arc"):
        run([(0, 3, 1.0)], value=1.0)
    with pytest.raises(AssertionError):
        run([(0, 1, 0.0)], value=0.0)   # an entry must carry flow > 0


def test_checker_rejects_a_non_maximal_flow():
    bad = [(0, 1, 12.0), (1, 3, 12.0), (3, 5, 12.0)]
    with pytest.raises(AssertionError, match="not maximal"):
        run(bad, value=12.0)
    with pytest.raises(AssertionError, match="value"):
        run(FLOW, value=22.0)


def test_checker_rejects_flow_in_both_directions_of_a_pair():
    # 1 -> 2 and 2 -> 1 both exist in C; 3 units circulating between them keep conservation but break the single-direction rule
    bad = [(0, 1, 12.0), (0, 2, 11.0), (1, 2, 3.0), (1, 3, 12.0), (2, 1, 3.0), (2, 4, 11.0), (3, 5, 19.0), (4, 3, 7.0), (4, 5, 4.0)]
    with pytest.raises(AssertionError, match="both"):
        run(bad)


def test_checker_rejects_unsorted_entries():
    with pytest.raises(AssertionError, match="sorted"):
        run(FLOW[::-1])


def test_value_solver_on_hand_cases():
    assert dinic(6, ROWS, COLS, CAPS, 0, 5) == 23.0
    assert dinic(2, [0], [1], [2.5], 0, 1) == 2.5
    assert dinic(2, [0], [1], [2.5], 1, 0) == 0.0
    # diagonal, zero, -0.0 and negative entries carry nothing
    assert dinic(3, [0, 0, 1, 1, 0], [0, 1, 2, 1, 2], [9.0, 3.0, -0.0, 4.0, -2.0], 0, 2) == 0.0
    # a path with a bottleneck in the middle; two disjoint paths; an antiparallel pair on a cycle through src
    n = 9
    caps = np.full(n - 1, 10.0)
    caps[4] = 3.0
    assert dinic(n, np.arange(n - 1), np.arange(1, n), caps, 0, n - 1) == 3.0
    assert dinic(4, [0, 0, 1, 2], [1, 2, 3, 3], [1.0, 2.0, 3.0, 1.0], 0, 3) == 2.0
    assert dinic(4, [0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 3, 2], [5.0, 7.0, 2.0, 9.0, 6.0, 1.0], 0, 3) == 3.0


def test_value_solver_equals_the_min_cut_by_enumeration():
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(3, 8))
        m = int(rng.integers(n, 3 * n))
        key = np.unique(rng.integers(0, n * n, m))
        rows, cols = key // n, key % n
        caps = rng.integers(-1, 9, len(key)).astype(np.float64)
        best = None
        for mask in range(1 << n):   # every cut with src inside and sink outside
            if not (mask & 1) or (mask >> (n - 1)) & 1:
                continue
            cut = sum(c for u, v, c in zip(rows, cols, caps) if u != v and c > 0 and (mask >> u) & 1 and not (mask >> v) & 1)
            best = cut if best is None or cut < best else best
        assert dinic(n, rows, cols, caps, 0, n - 1) == best


def test_fgpu_maxflow_is_declared_and_bound_alike():
    from falkordb_amd import _ffi
    with open(os.path.join(ROOT, "include", "fgpu.h")) as f:
        text = f.read()
    m = re.search(r"fgpu_info\s+fgpu_maxflow\s*\(([^;]*)\)\s*;", text)
    assert m, "include/fgpu.h does not declare fgpu_maxflow"
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert "fgpu_maxflow" in _ffi.SIGNATURES
    restype, argtypes = _ffi.SIGNATURES["fgpu_maxflow"]
    assert len(argtypes) == len(params) == 10
