"""CPU: the betweenness checker of tests/bc_check.py against networkx and hand graphs, and algo.betweenness' source rule
(fh_betweenness_sources) against a Python restatement of algo_procedures.rs:898-975."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bc_check import betweenness, csr_of  # noqa: E402


def bc(n, rows, cols, sources, active=None, batch=16):
    rp, ci = csr_of(n, rows, cols)
    return betweenness(n, rp, ci, sources, active, batch)[0]


@pytest.mark.parametrize("seed", range(8))
def test_checker_matches_networkx(seed):
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 120))
    m = int(rng.integers(0, 4 * n))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from((int(a), int(b)) for a, b in zip(rows, cols) if a != b)
    srcs = sorted(set(rng.choice(n, int(rng.integers(1, n + 1)), replace=True).tolist()))
    want = nx.betweenness_centrality_subset(g, srcs, list(range(n)), normalized=False)
    for batch in (16, 3):
        got = bc(n, rows, cols, srcs, batch=batch)
        assert np.allclose(got, [want[v] for v in range(n)], rtol=1e-12, atol=1e-12)


def test_hand_graphs():
    # the reference's test_betweenness_centrality graph: A->B, B->C, B->D, C->E, D->E, all five sources
    assert bc(5, [0, 1, 1, 2, 3], [1, 2, 3, 4, 4], range(5)).tolist() == [0, 3, 1, 1, 0]
    # a path 0 -> 1 -> ... -> 5: vertex i lies on i * (5 - i) source / target pairs
    assert bc(6, range(5), range(1, 6), range(6)).tolist() == [i * (5 - i) for i in range(6)]
    # a star out of 0 and a star into 0: no vertex lies between two others
    assert bc(6, [0] * 5, range(1, 6), range(6)).tolist() == [0] * 6
    assert bc(6, range(1, 6), [0] * 5, range(6)).tolist() == [0] * 6
    # a diamond 0 -> {1, 2} -> 3 -> 4: sigma(3) = 2, each side carries half of 0's paths to 3 and 4
    assert bc(5, [0, 0, 1, 2, 3], [1, 2, 3, 3, 4], [0]).tolist() == [0, 1, 1, 1, 0]
    # self-loops and duplicate entries change nothing
    assert bc(5, [0, 0, 0, 1, 2, 3, 3, 3], [0, 1, 1, 3, 3, 4, 3, 4], [0]).tolist() == bc(5, [0, 1, 3], [1, 3, 4], [0]).tolist()
    # a duplicate source counts twice; no sources give zeros
    assert bc(5, [0, 0, 1, 2, 3], [1, 2, 3, 3, 4], [0, 0]).tolist() == [0, 2, 2, 2, 0]
    assert bc(5, [0, 1], [1, 2], []).tolist() == [0] * 5


def test_active_mask_is_an_induced_subgraph():
    act = np.array([True, True, False, True, True])
    # 0 -> 1 -> 2 -> 3 and 1 -> 3 -> 4: with 2 gone, 1 still reaches 3 directly
    got = bc(5, [0, 1, 2, 1, 3], [1, 2, 3, 3, 4], [0, 1, 3, 4], act)
    assert got.tolist() == [0, 2, 0, 2, 0]


def _sources_ref(n_nodes, size, seed):
    """algo_procedures.rs:898-975, restated"""
    if size <= 0:
        raise ValueError("samplingSize must be a positive integer")
    size = ((size & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000          # `as i32`
    size &= 0xFFFFFFFFFFFFFFFF                                        # `as usize`
    seed &= 0xFFFFFFFFFFFFFFFF                                        # `as u64`
    if n_nodes == 0:
        return []
    if size >= n_nodes:
        return list(range(n_nodes))
    out, used, rng = [], set(), seed
    for i in range(size):
        if seed == 0:
            idx = i % n_nodes
        else:
            rng = (rng * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
            idx = (rng >> 33) % n_nodes
        if idx not in used:
            used.add(idx)
            out.append(idx)
    return out


@pytest.mark.parametrize("n_nodes,size,seed", [
    (100, 16, 0), (10, 16, 0), (16, 16, 0), (17, 16, 0), (1, 1, 0), (0, 16, 0),
    (1000, 16, 10), (1000, 300, 231231), (5, 3, 231231), (5, 3, 100), (7, 40, 5),
    (1000, 16, -1), (1000, 50, -(1 << 63)), (50, 49, 12345),              # negative seeds wrap; repeats dropped
    (100, (1 << 32) + 5, 0), (100, (1 << 32) + 5, 9), (100, 1 << 31, 3), (100, 1 << 32, 0), (100, (1 << 62) + 7, 11),
])
def test_source_rule(n_nodes, size, seed):
    want = _sources_ref(n_nodes, size, seed)
    got = host.betweenness_sources(n_nodes, size, seed).tolist()
    assert got == want


def test_source_rule_cases_named_by_the_issue():
    assert host.betweenness_sources(100, (1 << 32) + 5, 0).tolist() == [0, 1, 2, 3, 4]   # 2^32 + 5 means 5
    assert host.betweenness_sources(100, 1 << 31, 7).tolist() == list(range(100))        # 2^31: all nodes
    got = host.betweenness_sources(6, 5, 231231).tolist()
    assert len(got) == len(set(got)) and len(got) < 5                                     # a repeat was dropped
    for bad in (0, -21, -(1 << 40)):
        with pytest.raises(host.HostError) as e:
            host.betweenness_sources(10, bad, 0)
        assert "samplingSize must be a positive integer" in str(e.value)
