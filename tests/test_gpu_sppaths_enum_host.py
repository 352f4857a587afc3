"""GPU: every shape of algo.SPpaths and algo.SSpaths through the host layer (fh_algo_sp_paths_rows / fh_algo_ss_paths) against
the checker of tests/sppaths_enum_check.py: the reference's own cases (tests/golden/sppaths_enum_flow.json), seeded random
multigraphs on which the rows must be the checker's sequence exactly — relationship lists, nodes, weight and cost bit patterns —
with and without the pruning table of fgpu_sssp_hops, the deep_search fixture's step counts, the fgpu_sssp fallback, the fast
shape and the errors.  max_examined is set in every call: a regression ends in an exception, not in a hang."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sppaths_enum_check as K  # noqa: E402
from test_sppaths_enum_cpu import FLOW, expect, golden_call, golden_graph  # noqa: E402

pytestmark = pytest.mark.gpu
BUDGET = 2_000_000
F64 = np.float64


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def build(hctx, n, edges, order, deleted=()):
    g = host.Graph(hctx, max(n, 1))
    tid = {t: g.add_type(t) for t in order}
    if len(edges) > 1000:   # (the 3000-vertex fixture: one batch per type instead of 24 000 calls)
        for t in order:
            mine = [e for e in edges if e[1] == t]
            g.create_edges(tid[t], [e[2] for e in mine], [e[3] for e in mine], [e[0] for e in mine])
        g.commit()
    else:
        for i, t, s, d in edges:
            g.create_edge(tid[t], s, d, i)
    for v in deleted:
        g.delete_node(v)
    return g


def bits(x):
    return F64(x).view(np.uint64)


def same(got, want):
    """the host layer's rows against the checker's: the same sequence, bit for bit"""
    assert len(got) == len(want)
    for (nodes, rels, w, c), (we, wn, ww, wc) in zip(got, want):
        assert list(map(int, rels)) == we and list(map(int, nodes)) == wn
        assert bits(w) == bits(ww) and bits(c) == bits(wc)


@pytest.fixture(scope="module")
def golden_graphs(hctx):
    built = {}

    def get(case):
        key = case.get("branchy") or repr((case["nodes"], case["edges"]))
        if key not in built:
            n, edges, order, _, _ = golden_graph(case)
            built[key] = build(hctx, n, edges, order)
        return built[key]
    return get


@pytest.mark.parametrize("case", FLOW["cases"], ids=lambda c: c["name"])
def test_reference_cases(hctx, golden_graphs, case):
    g = golden_graphs(case)
    (edges, order, n, source, target), kw = golden_call(case)
    if target is None:
        got = g.algo_ss_paths(source, max_examined=BUDGET, **kw)
        expect(case, [(list(r[1]), list(r[0]), r[2], r[3]) for r in got])
        same(got, K.paths(edges, order, n, source, None, **kw))
        return
    got, st = g.algo_sp_paths_rows(source, target, max_examined=BUDGET, stats=True, **kw)
    expect(case, [(list(r[1]), list(r[0]), r[2], r[3]) for r in got])
    want_st = {}
    want = K.paths(edges, order, n, source, target, prune=True, stats=want_st, **kw)
    same(got, want)
    assert st == want_st
    if case.get("branchy") == "3000x8" and kw["max_len"] > 5:
        return   # (the unpruned walk of these takes 294 000 steps: seconds on the host; maxLen 5 stands for them)
    plain, pst = g.algo_sp_paths_rows(source, target, prune=False, max_examined=BUDGET, stats=True, **kw)
    same(plain, want)
    assert st["examined"] <= pst["examined"] and pst["table_rows"] == -1


@pytest.mark.parametrize("seed", K.SEEDS)
def test_seeded_multigraphs(hctx, seed):
    n, edges, weights, costs = K.seeded_graph(seed)
    g = build(hctx, n, edges, ["R", "S"], deleted=[n - 1])
    for source, target, kw in K.seeded_calls(seed):
        kw = dict(kw, weights=weights, costs=costs)
        got, st = g.algo_sp_paths_rows(source, target, max_examined=BUDGET, stats=True, **kw)
        if K.is_fast_shape(source, target, kw):   # the fast shape returns what algo_sp_paths returns
            one = g.algo_sp_paths(source, target, kw["types"], kw["direction"], weights, costs)
            assert (one is None) == (len(got) == 0) and st["table_rows"] == 0
            if one is not None:
                assert list(got[0][0]) == list(one[0]) and list(got[0][1]) == list(one[1])
                assert bits(got[0][2]) == bits(one[2]) and bits(got[0][3]) == bits(one[3])
        else:
            a, b = {}, {}
            same(got, K.paths(edges, ["R", "S"], n, source, target, prune=True, stats=b, deleted=(n - 1,), **kw))
            assert st == b, (source, target, kw)
            plain, pst = g.algo_sp_paths_rows(source, target, prune=False, max_examined=BUDGET, stats=True, **kw)
            same(plain, K.paths(edges, ["R", "S"], n, source, target, prune=False, stats=a, deleted=(n - 1,), **kw))
            assert pst == a and st["examined"] <= pst["examined"]
        same(g.algo_ss_paths(source, max_examined=BUDGET, **kw), K.paths(edges, ["R", "S"], n, source, None, **kw))


def deep_case(name):
    return next(c for c in FLOW["cases"] if c["name"] == name)


def test_deep_search_prunes_to_under_one_percent(hctx, golden_graphs):
    case = deep_case("10_deep_7_88_maxLen_5_pathCount_0")
    g = golden_graphs(case)
    (_, _, _, source, target), kw = golden_call(case)
    rows, st = g.algo_sp_paths_rows(source, target, max_examined=BUDGET, stats=True, **kw)
    plain, pst = g.algo_sp_paths_rows(source, target, prune=False, max_examined=BUDGET, stats=True, **kw)
    print("examined with pruning", st["examined"], "without", pst["examined"])
    assert [len(r[1]) for r in rows] == [4, 4] and st["table_rows"] == 6
    assert [list(r[1]) for r in plain] == [list(r[1]) for r in rows]
    assert st["examined"] * 100 < pst["examined"]


def test_deep_search_is_decided_by_the_table_alone(hctx, golden_graphs):
    case = deep_case("10_deep_1_137_maxLen_5_pathCount_0")
    (_, _, _, source, target), kw = golden_call(case)
    rows, st = golden_graphs(case).algo_sp_paths_rows(source, target, max_examined=BUDGET, stats=True, **kw)
    assert rows == [] and st["examined"] == 0 and st["table_rows"] == 6


@pytest.mark.parametrize("max_len", [33, None])
def test_fallback_to_the_unbounded_distances(hctx, max_len):
    n, edges, weights, costs = K.seeded_graph(2)
    g = build(hctx, n, edges, ["R", "S"], deleted=[n - 1])
    hit = 0
    for source, target, kw in K.seeded_calls(2):
        kw = dict(kw, weights=weights, costs=costs, max_len=max_len, path_count=0)
        want_st, plain_st = {}, {}
        want = K.paths(edges, ["R", "S"], n, source, target, prune=True, stats=want_st, deleted=(n - 1,), **kw)
        assert want == K.paths(edges, ["R", "S"], n, source, target, prune=False, stats=plain_st, deleted=(n - 1,), **kw)
        got, st = g.algo_sp_paths_rows(source, target, max_examined=BUDGET, stats=True, **kw)
        same(got, want)
        assert st == want_st and (source == target or target == n - 1 or st["table_rows"] == 0)
        plain, pst = g.algo_sp_paths_rows(source, target, prune=False, max_examined=BUDGET, stats=True, **kw)
        same(plain, want)
        assert pst == plain_st and st["examined"] <= pst["examined"]
        hit += len(got) > 0
    assert hit >= 3


@pytest.mark.parametrize("max_len", [32, 33, 34, 35, None])
@pytest.mark.parametrize("path_count", [0, 1, 2])
def test_hop_limited_optimum_heavier_than_the_unbounded_one(hctx, max_len, path_count):
    # chain 0 -> ... -> 35 at 1.0 each plus 0 -> 35 at 100.0: under maxLen 33 and 34 only the heavy arc qualifies, while
    # fgpu_sssp's one row (the fallback beyond 32 hops) says 35.0 — it may prune, it must not seed the bound
    n, edges, weights = K.detour_graph()
    g = build(hctx, n, edges, ["R"])
    kw = dict(weights=weights, max_len=max_len, path_count=path_count)
    want_st = {}
    want = K.paths(edges, ["R"], n, 0, n - 1, prune=False, **kw)
    assert want == K.paths(edges, ["R"], n, 0, n - 1, prune=True, stats=want_st, **kw)
    short = max_len is not None and max_len < 35
    assert [r[2] for r in want] == ([100.0] if short else [35.0, 100.0] if path_count == 2 else [35.0])
    if max_len is None and path_count == 1:
        want_st = None   # (the fast shape)
    got, st = g.algo_sp_paths_rows(0, n - 1, max_examined=BUDGET, stats=True, **kw)
    same(got, want)
    assert want_st is None or st == want_st
    plain = g.algo_sp_paths_rows(0, n - 1, prune=False, max_examined=BUDGET, **kw)
    same(plain, want)
    # without the heavy arc the target is out of reach within maxLen 33, in reach without: no rows and no walk
    h = build(hctx, n, edges[:-1], ["R"])
    got, st = h.algo_sp_paths_rows(0, n - 1, weights=weights, max_len=33, path_count=path_count, max_examined=BUDGET, stats=True)
    assert got == [] and st["examined"] == 0 and st["table_rows"] == 0


def test_errors(hctx):
    edges = [(0, "R", 0, 1), (1, "R", 0, 2), (2, "R", 0, 3), (3, "R", 1, 4), (4, "R", 2, 4), (5, "R", 3, 4)]
    g = build(hctx, 5, edges, ["R"])
    assert [list(r[1]) for r in g.algo_sp_paths_rows(0, 4, path_count=2, max_len=3, max_examined=BUDGET)] == [[1, 4], [2, 5]]
    for who, call in (("SPpaths", lambda **kw: g.algo_sp_paths_rows(0, 4, **kw)), ("SSpaths", lambda **kw: g.algo_ss_paths(0, **kw))):
        with pytest.raises(host.HostError, match=who + ".*negative weight"):
            call(weights={1: -0.5}, max_len=3)
        with pytest.raises(host.HostError, match="non-negative integer"):
            call(path_count=-1)
        with pytest.raises(host.HostError, match="budget"):
            call(path_count=0, max_len=3, max_examined=2)
    with pytest.raises(host.HostError, match="negative weight"):
        g.algo_sp_paths_rows(0, 4, weights={1: -0.5})   # the fast shape
    assert len(g.algo_sp_paths_rows(0, 4, path_count=0, max_len=3, max_examined=BUDGET)) == 3   # the graph still answers
