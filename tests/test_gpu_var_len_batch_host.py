"""CondVarLenTraverseOp::expand_batch (host layer over fgpu_expand_trails) through fh_var_len_traverse_batch: equal, row by row
and in order, to the concatenation of var_len_traverse (the per-row DFS) over the same rows — which tests/test_gpu_host.py holds
against oracle.model.var_len_expand — and to the oracle itself."""
import numpy as np
import pytest

from falkordb_amd import host

from oracle import model
from test_gpu_host import _twin_graphs

pytestmark = pytest.mark.gpu
DIRECTIONS = ({}, {"reversed": True}, {"bidirectional": True})


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def per_row(g, starts, dests=None, **kw):
    rows, frames = [], 0
    for i, s in enumerate(starts):
        got, st = g.var_len_traverse(s, dest=None if dests is None else dests[i], **kw)
        rows += [(i, *r) for r in got]
        frames += st["frames"]
    return rows, frames


def oracle_rows(og, starts, dests=None, **kw):
    return [(i, *r) for i, s in enumerate(starts)
            for r in model.var_len_expand(og, s, dest=None if dests is None else dests[i], **kw)]


def twins(hctx, seed, commit):
    rng = np.random.default_rng(seed)
    n = 9
    edges = [(("KNOWS", "LIKES")[int(rng.integers(0, 2))], int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(16)]
    edges += [edges[0], edges[3]]                                  # multi-edge pairs
    return _twin_graphs(hctx, n, edges, [("L", v) for v in range(0, n, 2)], commit)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("commit", [True, False], ids=["committed", "pending-deltas"])
def test_batch_equals_the_rows_one_by_one(hctx, seed, commit):
    g, og = twins(hctx, seed, commit)
    starts = [0, 3, 7, 3, 8]
    for kw in DIRECTIONS:
        for (lo, hi) in ((1, 1), (1, 3), (2, 4), (0, 2)):
            args = dict(min_hops=lo, max_hops=hi, emit_path=True, **kw)
            want, frames = per_row(g, starts, prune=False, **args)
            got, st = g.var_len_traverse_batch(starts, **args)
            assert got == want == oracle_rows(og, starts, **args), (kw, lo, hi)
            assert st["device_calls"] == 1 and st["frames"] == frames and st["pruned"] == 0
            dests = [2, None, 7, 3, 2]
            want, _ = per_row(g, starts, dests, **args)
            got, st = g.var_len_traverse_batch(starts, dests, **args)
            assert got == want and st["device_calls"] == 1 and st["reach_products"] == 0, (kw, lo, hi)
        args = dict(types=["KNOWS"], max_hops=3, dst_labels=["L"], **kw)
        assert g.var_len_traverse_batch(starts, **args)[0] == per_row(g, starts, **args)[0] == oracle_rows(og, starts, **args)
        args = dict(types=["LIKES", "NOPE"], max_hops=2, **kw)                       # an unknown type is dropped
        assert g.var_len_traverse_batch(starts, **args)[0] == per_row(g, starts, **args)[0]
        args = dict(types=["NOPE", "LIKES"], max_hops=2, **kw)                       # the unknown name first
        assert g.var_len_traverse_batch(starts, **args)[0] == per_row(g, starts, **args)[0] == oracle_rows(og, starts, **args)
        args = dict(types=["KNOWS", "KNOWS"], max_hops=2, emit_path=True, **kw)      # a name listed twice is walked twice
        got = g.var_len_traverse_batch(starts, **args)[0]
        assert got == per_row(g, starts, **args)[0] == oracle_rows(og, starts, **args)
        assert len(got) > len(g.var_len_traverse_batch(starts, **dict(args, types=["KNOWS"]))[0])
        got, st = g.var_len_traverse_batch(starts, types=["NOPE"], min_hops=0, max_hops=2, **kw)   # none resolvable: the 0-hop rows
        assert got == [(i, s, s, None) for i, s in enumerate(starts)] and st["device_calls"] == 1
        got, st = g.var_len_traverse_batch(starts, max_hops=2, dst_labels=["MISSING"], **kw)
        assert got == [] and st["device_calls"] == 0                                 # a missing label: no rows, no device call


def test_host_rows_are_spliced_in_place(hctx):
    g, og = twins(hctx, 3, True)
    g.delete_node(4)
    starts = [0, 50, 3, 4, 7, 9]                                                     # 50 and 9: at or past the capacity; 4: deleted
    for kw in DIRECTIONS:
        args = dict(min_hops=0, max_hops=3, emit_path=True, **kw)
        want, _ = per_row(g, starts, **args)
        got, st = g.var_len_traverse_batch(starts, **args)
        assert got == want and st["device_calls"] == 1
        assert {r[0] for r in got} >= {0, 1, 2, 3, 4, 5}                              # every row has its 0-hop emission
        dests = [2, 2, 60, 3, 4, None]                                               # a dest out of range, a deleted dest
        want, _ = per_row(g, starts, dests, prune=False, **args)                     # (the reach sets take no dest past the capacity)
        assert g.var_len_traverse_batch(starts, dests, prune=False, **args)[0] == want
    got, st = g.var_len_traverse_batch([50, 9], min_hops=0, max_hops=2)              # nothing to send
    assert [r[:3] for r in got] == [(0, 50, 50), (1, 9, 9)] and st["device_calls"] == 0
    assert g.var_len_traverse_batch([], max_hops=2) == ([], {"frames": 0, "pruned": 0, "reach_products": 0, "device_calls": 0})


def test_small_budget_bisects_down_to_host_rows(hctx):
    g, og = twins(hctx, 1, True)
    starts = [0, 3, 7, 3, 8, 1, 2, 5]
    args = dict(min_hops=1, max_hops=3, emit_path=True, bidirectional=True)
    want, frames = per_row(g, starts, prune=False, **args)
    assert len(want) > 100
    got, st = g.var_len_traverse_batch(starts, **args)
    assert got == want and st["device_calls"] == 1
    got, st = g.var_len_traverse_batch(starts, device_budget=1, **args)              # not even one root fits: every row is the host's
    assert got == want and st["device_calls"] == 8 + 4 + 2 + 1 and st["frames"] == frames
    got, st = g.var_len_traverse_batch(starts, device_budget=len(want) // 2, **args)  # the batch does not fit, parts of it do
    assert got == want and 1 < st["device_calls"] <= 15 and st["frames"] == frames
    dests = [2] * 8
    want, _ = per_row(g, starts, dests, **args)
    got, st = g.var_len_traverse_batch(starts, dests, device_budget=1, **args)       # the host rows prune as set
    assert got == want and st["reach_products"] > 0


def test_symbol_is_declared_exported_and_bound():
    import os
    import subprocess
    from falkordb_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "fh_var_len_traverse_batch(" in open(os.path.join(root, "include", "falkor_host.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", build.HOST_LIB], capture_output=True, text=True, check=True).stdout
    assert " T fh_var_len_traverse_batch" in out
    assert callable(host.Graph.var_len_traverse_batch)
