"""GPU: fgpu_shortest_path_batch against the contract restated in tests/spath_check.py — the node list and all eight stats of
every query, by equality.  Every batch runs with the backward pattern given and left to the call unless a test says otherwise."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FGPU_DIM_MISMATCH, FGPU_INVALID, FGPU_NULL_POINTER, FGPU_OUT_OF_BOUNDS, FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spath_check import NO_MEET, prepare, search  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
HUB_DEG = 4096   # common.hpp


def same(got, want, what):
    path, st = got
    wpath, wst = want
    assert (None if path is None else path.tolist()) == wpath, f"{what}: path {path}, the checker says {wpath}"
    assert st == wst, f"{what}: stats {st}, the checker's {wst}"


def hold(ctx, n, rows, cols, queries, max_hops=(-1,), slots=(0,), undirected=False, F=None, given=(True, False)):
    """`queries` [(src, dst), ...] as one batch per (max_hops, slots, B given / NULL), every query against the checker (computed
    once per max_hops).  undirected: the pattern is S = F U F', passed for both sides.  Returns {(src, dst, max_hops): (path,
    stats)} as the checker has them."""
    rows, cols = np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64)
    if undirected:
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    own = F is None
    if own:
        F = ctx.mat_from_coo(n, n, rows, cols)
    B = F if undirected else F.transpose()
    tables = prepare(n, rows, cols)
    srcs, dsts = [s for s, _ in queries], [d for _, d in queries]
    out = {}
    try:
        for mh in max_hops:
            want = {q: search(tables, q[0], q[1], mh) for q in dict.fromkeys(queries)}
            for b in ((B,) if undirected else [B if g else None for g in given]):
                for sl in slots:
                    got = engine.shortest_path_batch(ctx, F, b, srcs, dsts, mh, sl, stats=True)
                    assert len(got) == len(queries)
                    for i, q in enumerate(queries):
                        same(got[i], want[q], f"query {i} {q} max_hops {mh} slots {sl} B {'given' if b else 'NULL'}")
            out.update({(q[0], q[1], mh): w for q, w in want.items()})
    finally:
        if not undirected:
            B.free()
        if own:
            F.free()
    return out


def test_parent_by_frontier_position_not_by_id(ctx):
    edges = [(0, 1), (0, 2), (1, 9), (2, 3), (9, 5), (3, 5), (5, 10), (5, 11), (5, 12), (10, 8), (11, 8), (12, 8)]
    got = hold(ctx, 13, [s for s, _ in edges], [d for _, d in edges], [(0, 8)], slots=(0, 1))
    assert got[(0, 8, -1)][0] == [0, 1, 9, 5, 10, 8]   # (an id-ordered frontier gives [0, 2, 3, 5, ...])


def test_side_by_vertex_count_not_by_entry_count(ctx):
    edges = [(0, 0), (0, 2), (0, 3), (1, 5), (2, 0), (2, 4), (3, 1), (4, 5)]
    got = hold(ctx, 6, [s for s, _ in edges], [d for _, d in edges], [(0, 5)], slots=(0, 1))
    assert got[(0, 5, -1)][0] == [0, 2, 4, 5]          # (the entry-count rule gives [0, 3, 1, 5])


def test_tied_candidates_the_first_key_is_the_meeting_vertex(ctx):
    got = hold(ctx, 4, [0, 0, 1, 2], [1, 2, 3, 3], [(0, 3)])
    assert got[(0, 3, -1)][0] == [0, 1, 3] and got[(0, 3, -1)][1][5:7] == [1, 2]
    # a fan of 70 two-hop routes: the backward side walks dst's row of 70 entries, all of them candidates, over two wavefronts;
    # the first key (rows ascend: the least id) is the meeting vertex
    k = 70
    mid = np.arange(2, k + 2)
    got = hold(ctx, k + 2, np.concatenate([np.zeros(k, dtype=np.int64), mid]), np.concatenate([mid, np.ones(k, dtype=np.int64)]),
               [(0, 1)])
    assert got[(0, 1, -1)][0] == [0, 2, 1] and got[(0, 1, -1)][1][6] == k


@pytest.mark.parametrize("width", [65, 257, 4097])
def test_frontier_order_across_wavefronts_and_workgroups(ctx, width):
    """s -> width vertices (ids permuted so that frontier order is not id order two levels on) -> one entry each -> a second
    layer -> t: every route has the same length, so any reordering of a frontier shows as another path"""
    rng = np.random.default_rng(width)
    s, t = 0, 1
    a = 2 + np.arange(width)                       # first layer, walked in id order
    b = 2 + width + rng.permutation(width)         # second layer: a[i] -> b[i], so its frontier order is the permutation
    c = 2 + 2 * width + rng.permutation(width)     # third layer: b[i] -> c[i]
    d = 2 + 3 * width + np.arange(width)           # fourth: c[i] -> d[i] -> t
    rows = np.concatenate([np.full(width, s), a, b, c, d])
    cols = np.concatenate([a, b, c, d, np.full(width, t)])
    n = 2 + 4 * width
    got = hold(ctx, n, rows, cols, [(s, t), (int(a[3]), t), (s, int(d[5]))], slots=(0, 1))
    path = got[(s, t, -1)][0]
    assert len(path) == 6 and got[(s, t, -1)][1][0] + got[(s, t, -1)][1][1] == 5
    hold(ctx, n, rows, cols, [(s, t), (t, s)], undirected=True)


@pytest.mark.parametrize("role", ["src", "dst", "middle"])
def test_hub_row_beside_ten_one_entry_rows(ctx, role):
    k = 5000
    assert k > HUB_DEG
    hub, a, b = 0, k + 1, k + 2
    leaves = np.arange(1, k + 1)
    chain = np.arange(k + 3, k + 14)   # eleven vertices in a row: ten rows of one entry
    if role == "src":      # hub -> leaves -> b
        rows, cols = np.concatenate([np.full(k, hub), leaves]), np.concatenate([leaves, np.full(k, b)])
        q = [(hub, b), (hub, 77)]
    elif role == "dst":    # a -> leaves -> hub
        rows, cols = np.concatenate([np.full(k, a), leaves]), np.concatenate([leaves, np.full(k, hub)])
        q = [(a, hub), (4999, hub)]
    else:                  # a -> hub -> leaves -> b, and leaves -> hub
        rows = np.concatenate([[a], np.full(k, hub), leaves, leaves])
        cols = np.concatenate([[hub], leaves, np.full(k, b), np.full(k, hub)])
        q = [(a, b), (hub, b)]
    rows, cols = np.concatenate([rows, chain[:-1]]), np.concatenate([cols, chain[1:]])
    small = [(int(chain[i]), int(chain[i + 1])) for i in range(10)]
    queries = small[:5] + q[:1] + small[5:] + q[1:] + [(int(chain[0]), int(chain[10]))]
    got = hold(ctx, k + 14, rows, cols, queries, max_hops=(-1, 1), slots=(64,))
    assert got[(q[0][0], q[0][1], -1)][0] is not None and got[(q[0][0], q[0][1], -1)][1][4] >= k


def test_groups_agree_with_one_slot(ctx):
    R = ctx.mat_rmat(10)
    n = R.nrows
    rp, ci, _ = R.export_csr()
    rows, cols = np.repeat(np.arange(n), np.diff(rp.astype(np.int64))), ci.astype(np.int64)
    live = np.nonzero(np.diff(rp.astype(np.int64)))[0]
    rng = np.random.default_rng(5)
    pairs = [(int(s), int(d)) for s, d in rng.choice(live, (20, 2))]
    pairs[7] = pairs[2]                                       # a duplicate
    pairs += [(pairs[0][0], int(d)) for d in live[:6]]        # the same src with other dsts: later groups meet its reset ball
    one = engine.shortest_path_batch(ctx, R, None, [s for s, _ in pairs], [d for _, d in pairs], slots=1, stats=True)
    assert any(p is not None for p, _ in one)

    def agree(qs, sl, ref):
        got = engine.shortest_path_batch(ctx, R, None, [s for s, _ in qs], [d for _, d in qs], slots=sl, stats=True)
        for i, (g, w) in enumerate(zip(got, ref)):
            assert (g[0] is None) == (w[0] is None) and (g[0] is None or np.array_equal(g[0], w[0])) and g[1] == w[1], (sl, i, qs[i])

    for sl in (2, 64, 0, len(pairs) - 1):                     # count = slots + 1: a last group of one
        agree(pairs, sl, one)
    perm = rng.permutation(len(pairs))
    agree([pairs[i] for i in perm], 3, [one[i] for i in perm])
    same_q = [pairs[0]] * 9                                   # the same query on both sides of a group boundary
    agree(same_q, 4, [one[0]] * 9)
    hold(ctx, n, rows, cols, pairs, slots=(3,), F=R, given=(False,))
    R.free()


def test_one_group_mixes_a_long_path_one_hop_unreachable_and_src_equals_dst(ctx):
    n = 44
    rows, cols = list(range(40)) + [41], list(range(1, 41)) + [42]   # a path of 40 hops, a separate edge, 43 isolated
    got = hold(ctx, n, rows, cols, [(0, 40), (10, 11), (5, 42), (7, 7), (41, 42), (40, 0), (0, 43), (43, 0)], slots=(0, 3))
    assert len(got[(0, 40, -1)][0]) == 41
    assert got[(5, 42, -1)][0] is None and got[(7, 7, -1)] == (None, [0, 0, 0, 0, 0, NO_MEET, 0, 0])
    assert got[(43, 0, -1)][1][:2] == [1, 0]   # a seed without entries is a level all the same


@pytest.mark.parametrize("L", [1, 2, 5])
def test_max_hops_around_the_length(ctx, L):
    rows, cols = list(range(L)), list(range(1, L + 1))
    got = hold(ctx, L + 2, rows, cols, [(0, L), (L, 0), (0, L + 1)], max_hops=(L - 1, L, 0, -1, L + 1))
    assert got[(0, L, L)][0] == list(range(L + 1)) and got[(0, L, -1)][0] == list(range(L + 1))
    assert got[(0, L, L - 1)][0] is None and got[(0, L, 0)][0] is None


def test_undirected_with_reciprocal_edges_and_self_loops(ctx):
    rng = np.random.default_rng(11)
    n = 90
    rows, cols = rng.integers(0, n, 150), rng.integers(0, n, 150)
    rows, cols = np.concatenate([rows, cols[:20], np.arange(0, n, 9)]), np.concatenate([cols, rows[:20], np.arange(0, n, 9)])
    queries = [(int(s), int(d)) for s, d in rng.integers(0, n, (60, 2))]
    got = hold(ctx, n, rows, cols, queries, max_hops=(-1, 3), slots=(0, 7), undirected=True)
    assert sum(p is not None for p, _ in got.values()) > 20
    hold(ctx, n, rows, cols, queries, max_hops=(-1,), slots=(0, 7))


def test_hypersparse_pattern(ctx):
    n = 100_000
    rows, cols = np.array([7, 99_999, 50_000, 7], dtype=U64), np.array([99_999, 50_000, 7, 12], dtype=U64)
    order = np.lexsort((cols, rows))
    r, c = rows[order], cols[order]
    hrows, cnt = np.unique(r, return_counts=True)
    H = ctx.mat_from_csr(n, n, np.concatenate([[0], np.cumsum(cnt)]).astype(U64), c, hyper_rows=hrows.astype(U64))
    got = hold(ctx, n, rows, cols, [(7, 50_000), (50_000, 50_000), (50_000, 99_999), (3, 7), (12, 7)], max_hops=(-1, 1), F=H)
    H.free()
    assert got[(7, 50_000, -1)][0] == [7, 99_999, 50_000]


@pytest.mark.parametrize("n", [65, 127])
def test_odd_vertex_counts_and_the_reset(ctx, n):
    # two routes of equal length between the first and the last vertex, through the highest ids
    rows, cols = [0, 0, n - 2, n - 3], [n - 2, n - 3, n - 1, n - 1]
    queries = [(0, n - 1), (n - 1, 0), (n - 1, n - 1), (0, n - 1), (0, n - 2), (0, n - 1), (n - 3, n - 1), (0, n - 1)]
    got = hold(ctx, n, rows, cols, queries, max_hops=(-1, 2, 1), slots=(3,))
    assert got[(0, n - 1, -1)][0] == [0, n - 3, n - 1]


@pytest.mark.parametrize("symmetric", [False, True])
def test_rmat_14_two_hundred_pairs(ctx, symmetric):
    R = ctx.mat_rmat(14)
    n = R.nrows
    rp, ci, _ = R.export_csr()
    rows, cols = np.repeat(np.arange(n), np.diff(rp.astype(np.int64))), ci.astype(np.int64)
    live = np.nonzero(np.diff(rp.astype(np.int64)))[0]
    pairs = [(int(s), int(d)) for s, d in np.random.default_rng(0xB7C).choice(live, (200, 2))]
    got = hold(ctx, n, rows, cols, pairs, undirected=symmetric, F=None if symmetric else R, given=(False,))
    R.free()
    assert sum(p is not None for p, _ in got.values()) > 100
    assert any(st[0] and st[1] for _, st in got.values())   # both balls grew in some query


def test_two_calls_return_identical_arrays_and_three_threads_agree(ctx):
    A = ctx.mat_rmat(12)
    At = A.transpose()
    n = A.nrows
    rp, _, _ = A.export_csr()
    live = np.nonzero(np.diff(rp.astype(np.int64)))[0]
    srcs, dsts = [int(v) for v in live[:40]], [int(v) for v in live[40:80]]
    a = engine.shortest_path_batch(ctx, A, None, srcs, dsts, stats=True)
    b = engine.shortest_path_batch(ctx, A, None, srcs, dsts, stats=True)
    assert any(p is not None for p, _ in a)

    def equal(x, y):
        return all((p is None) == (q is None) and (p is None or np.array_equal(p, q)) and s == t for (p, s), (q, t) in zip(x, y))
    assert equal(a, b)
    results, errors = {}, []

    def batch(k):
        try:
            results[k] = engine.shortest_path_batch(ctx, A, At if k % 2 else None, srcs, dsts, slots=(0, 5, 64)[k], stats=True)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=batch, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    At.free()
    A.free()
    assert not errors, errors
    assert all(equal(a, results[k]) for k in range(3))


def test_arguments(ctx):
    A = ctx.mat_from_coo(4, 4, np.array([0, 1], dtype=U64), np.array([1, 2], dtype=U64))
    R = ctx.mat_from_coo(4, 5, np.array([0], dtype=U64), np.array([1], dtype=U64))
    assert engine.shortest_path_batch(ctx, A, None, [], []) == []
    none = np.zeros(0, dtype=U64)
    for n in (1, 65):
        E = ctx.mat_from_coo(n, n, none, none)
        got = engine.shortest_path_batch(ctx, E, None, [0, n - 1, 0], [n - 1, 0, 0], stats=True)
        level = 1 if n > 1 else 0   # (n == 1: src == dst)
        assert got == [(None, [level, 0, 0, 0, 0, NO_MEET, 0, 0])] * 2 + [(None, [0, 0, 0, 0, 0, NO_MEET, 0, 0])]
        E.free()
    # an index out of range in the middle of a batch: refused before any work, the outputs untouched
    for srcs, dsts in (([0, 4, 1], [2, 0, 2]), ([0, 0, 1], [2, 2**40, 2])):
        with pytest.raises(FgpuError) as e:
            engine.shortest_path_batch(ctx, A, None, srcs, dsts)
        assert e.value.code == FGPU_OUT_OF_BOUNDS and "query 1" in str(e.value)
    u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)

    def raw(F, B, s, d, slots=0, length=True, off=True, nodes_out=True):
        s, d = np.asarray(s, dtype=U64), np.asarray(d, dtype=U64)
        ln, of, st = np.full(3, 77, dtype=np.int64), np.full(4, 77, dtype=U64), np.full(24, 77, dtype=U64)
        nodes = u64p()
        code = ctx.lib.fgpu_shortest_path_batch(ctx._h, F, B, s.ctypes.data_as(u64p) if len(s) else None,
                                                d.ctypes.data_as(u64p) if len(d) else None, C.c_uint64(3), C.c_int64(-1),
                                                C.c_uint32(slots), ln.ctypes.data_as(i64p) if length else None,
                                                of.ctypes.data_as(u64p) if off else None, C.byref(nodes) if nodes_out else None,
                                                st.ctypes.data_as(u64p))
        assert (ln == 77).all() and (of == 77).all() and (st == 77).all() and not nodes, "an output was written on failure"
        return code
    ok = ([0, 1, 0], [2, 2, 1])
    assert raw(A._h, None, [0, 4, 1], [2, 0, 2]) == FGPU_OUT_OF_BOUNDS
    assert raw(None, None, *ok) == FGPU_NULL_POINTER
    assert raw(A._h, None, [], ok[1]) == FGPU_NULL_POINTER and raw(A._h, None, ok[0], []) == FGPU_NULL_POINTER
    assert raw(A._h, None, *ok, length=False) == FGPU_NULL_POINTER and raw(A._h, None, *ok, off=False) == FGPU_NULL_POINTER
    assert raw(A._h, None, *ok, nodes_out=False) == FGPU_NULL_POINTER
    assert raw(R._h, None, *ok) == FGPU_DIM_MISMATCH and raw(A._h, R._h, *ok) == FGPU_DIM_MISMATCH
    assert raw(A._h, None, *ok, slots=65) == FGPU_INVALID
    got = engine.shortest_path_batch(ctx, A, None, [0, 0], [2, 3], slots=64, stats=True)
    assert got[0][0].tolist() == [0, 1, 2] and got[1][0] is None
    A.free()
    R.free()
