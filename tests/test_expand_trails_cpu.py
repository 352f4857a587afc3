"""The placement rule of fgpu_expand_trails (tests/trails_check.py: level-synchronous expansion, E / S / base by sums and prefix
sums) against the reference's LIFO DFS (oracle.model.var_len_expand).  No GPU: this pins the rule the kernels implement."""
import numpy as np
import pytest

from oracle import model
from trails_check import graph_of, level_expand, random_multigraph

DIRECTIONS = ({}, {"reversed": True}, {"bidirectional": True})
HOPS = ((1, 1), (1, 3), (2, 4), (0, 2), (0, 0), (3, 2))


@pytest.mark.parametrize("seed", range(8))
def test_level_rule_equals_lifo_dfs_on_random_multigraphs(seed):
    rng = np.random.default_rng(seed)
    g, _ = random_multigraph(rng)
    rows = 0
    for start in (0, 3, 7):
        for kw in DIRECTIONS:
            for (lo, hi) in HOPS:
                for dest in (None, 2, start):
                    want = model.var_len_expand(g, start, dest=dest, min_hops=lo, max_hops=hi, emit_path=True, **kw)
                    assert level_expand(g, start, dest=dest, min_hops=lo, max_hops=hi, emit_path=True, **kw) == want, (start, kw, lo, hi, dest)
                    rows += len(want)
            for extra in ({"types": ["KNOWS"], "dst_labels": ["L"]}, {"types": ["LIKES", "NOPE", "KNOWS", "LIKES"]},
                          {"dst_labels": ["MISSING"], "min_hops": 0}, {"types": ["NOPE"], "min_hops": 0}):
                args = {"max_hops": 3, **extra, **kw}
                assert level_expand(g, start, **args) == model.var_len_expand(g, start, **args), (start, args)
    assert rows > 100


@pytest.mark.parametrize("seed", range(4))
def test_level_rule_unbounded_on_acyclic_graphs(seed):
    g, _ = random_multigraph(np.random.default_rng(100 + seed), acyclic=True)
    for start in (0, 1, 4):
        for kw in ({}, {"reversed": True}):
            for dest in (None, 5, start):
                want = model.var_len_expand(g, start, dest=dest, min_hops=1, max_hops=None, emit_path=True, **kw)
                assert level_expand(g, start, dest=dest, min_hops=1, max_hops=None, emit_path=True, **kw) == want


def test_level_rule_on_trail_shapes():
    tri = graph_of(3, [("R", 0, 1), ("R", 1, 2), ("R", 2, 0)])
    par = graph_of(2, [("R", 0, 1), ("R", 0, 1)])
    loop = graph_of(2, [("R", 0, 0), ("R", 0, 1)])
    for g in (tri, par, loop):
        for kw in DIRECTIONS:
            for start in range(g.n):
                want = model.var_len_expand(g, start, min_hops=0, max_hops=None, emit_path=True, **kw)
                assert want and level_expand(g, start, min_hops=0, max_hops=None, emit_path=True, **kw) == want
