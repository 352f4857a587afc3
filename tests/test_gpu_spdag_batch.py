"""GPU: fgpu_shortest_dag_batch against fgpu_shortest_dag on the same handles — length, the three arrays and the eight stats of
every query — and against the one-sided checker of tests/asp_check.py.  Every batch runs under spdag_sides 0 .. 3 and with the
transpose given and left to the call unless a test says otherwise; every comparison is array equality."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FGPU_INVALID, FGPU_OUT_OF_BOUNDS, FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asp_check import prepare, shortest_dag  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
HUB_DEG = 4096       # common.hpp
SD_SORT_MAX = 4096   # spdag.hpp
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asp_flow.json")))


def same_as_checker(got, want, what):
    L, f, t, d = got[:4]
    wl, wp = want
    assert L == wl, f"{what}: length {L}, the checker says {wl}"
    w = np.asarray(wp, dtype=U64).reshape(-1, 3)
    assert np.array_equal(f, w[:, 0]) and np.array_equal(t, w[:, 1]), f"{what}: the pairs differ from the checker's"
    assert np.array_equal(d, w[:, 2]), f"{what}: the depths differ from the checker's"


def same_as_single(got, one, what):
    assert got[0] == one[0], f"{what}: length {got[0]}, the single call says {one[0]}"
    for k, name in ((1, "from"), (2, "to"), (3, "depth")):
        assert np.array_equal(got[k], one[k]), f"{what}: {name} differs from the single call's"
    assert got[4] == one[4], f"{what}: stats {got[4]}, the single call's {one[4]}"


def hold(ctx, n, rows, cols, queries, max_hops=(-1,), slots=(0,), sides=(0, 1, 2, 3), A=None, checked=None):
    """`queries` [(src, dst), ...] as one batch per (max_hops, slots, spdag_sides, At given / None): every query against the
    single call on the same handles (computed once per setting) and the first `checked` (None: all) against the checker.
    Returns {(src, dst, max_hops): stats under spdag_sides 0 with At}."""
    rows, cols = np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64)
    own = A is None
    if own:
        A = ctx.mat_from_coo(n, n, rows, cols)
    At = A.transpose()
    prep = prepare(n, rows, cols)
    srcs, dsts = [s for s, _ in queries], [d for _, d in queries]
    distinct = list(dict.fromkeys(queries))
    stats = {}
    try:
        for mh in max_hops:
            want = {q: shortest_dag(n, None, None, q[0], q[1], mh, prepared=prep)
                    for q in list(dict.fromkeys(queries[:len(queries) if checked is None else checked]))}
            for sd in sides:
                ctx.set_option("spdag_sides", sd)
                for at in (At, None):
                    single = {q: engine.shortest_dag(ctx, A, at, q[0], q[1], mh, stats=True) for q in distinct}
                    for sl in slots:
                        got = engine.shortest_dag_batch(ctx, A, at, srcs, dsts, mh, sl, stats=True)
                        assert len(got) == len(queries)
                        for i, q in enumerate(queries):
                            what = f"query {i} {q} max_hops {mh} slots {sl} sides {sd} At {'given' if at else 'NULL'}"
                            same_as_single(got[i], single[q], what)
                            if q in want:
                                same_as_checker(got[i], want[q], what)
                            if sd == 0 and at is not None:
                                stats[(q[0], q[1], mh)] = got[i][4]
    finally:
        ctx.set_option("spdag_sides", 0)
        At.free()
        if own:
            A.free()
    return stats


@pytest.mark.parametrize("graph", ["acyclic", "cyclic"])
@pytest.mark.parametrize("symmetric", [False, True])
def test_golden_graphs_every_ordered_pair_in_one_batch(ctx, graph, symmetric):
    g = GOLD["graphs"][graph]
    n = len(g["nodes"])
    rows, cols = [s for s, _, _ in g["edges"]], [d for _, _, d in g["edges"]]
    if symmetric:
        rows, cols = rows + cols, cols + rows
    hold(ctx, n, rows, cols, [(s, d) for s in range(n) for d in range(n)], max_hops=(-1, 2), slots=(0, 1, 2, 3, 64))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_path_with_cut_and_uncut_queries_in_one_group(ctx, L):
    n = L + 3   # a tail behind L and an isolated vertex
    rows, cols = list(range(L + 1)), list(range(1, L + 2))
    queries = [(0, L), (L, 0), (1, L), (0, 0), (L + 1, 0), (0, L + 2), (L + 2, L + 2), (L + 2, 0), (0, L + 1), (L, L + 1)]
    st = hold(ctx, n, rows, cols, queries, max_hops=(-1, L, L - 1), slots=(64,))
    assert st[(0, L, -1)][0] + st[(0, L, -1)][1] == L and st[(0, L, -1)][6] == 1
    assert st[(0, L, L)][6] == 1 and st[(0, L, L - 1)][6] == 0


def test_repeated_query_across_the_group_boundary_and_permutation(ctx):
    # 0 -> {1, 2} -> 3 -> 4, 4 -> 0, 5 isolated
    rows, cols = [0, 0, 1, 2, 3, 4], [1, 2, 3, 3, 4, 0]
    hold(ctx, 6, rows, cols, [(0, 4)] * 65, slots=(0,))
    others = [(0, 3), (4, 4), (1, 0), (5, 0), (2, 4)]
    mixed = []
    for i in range(65):
        mixed.append((0, 4))
        if i % 13 == 0:
            mixed.append(others[i // 13])
    assert len(mixed) == 70
    hold(ctx, 6, rows, cols, mixed, slots=(0,))
    A = ctx.mat_from_coo(6, 6, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))
    fwd = engine.shortest_dag_batch(ctx, A, None, [s for s, _ in mixed], [d for _, d in mixed], stats=True)
    back = engine.shortest_dag_batch(ctx, A, None, [s for s, _ in mixed[::-1]], [d for _, d in mixed[::-1]], stats=True)
    A.free()
    for a, b in zip(fwd, back[::-1]):
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])) and a[4] == b[4]


@pytest.mark.parametrize("role", ["src", "dst", "middle"])
def test_hub_query_beside_ten_one_entry_rows(ctx, role):
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
    else:                  # a -> hub -> leaves -> b, and leaves -> hub (cycles of length 2 through the hub)
        rows = np.concatenate([[a], np.full(k, hub), leaves, leaves])
        cols = np.concatenate([[hub], leaves, np.full(k, b), np.full(k, hub)])
        q = [(a, b), (hub, hub)]
    rows, cols = np.concatenate([rows, chain[:-1]]), np.concatenate([cols, chain[1:]])
    small = [(int(chain[i]), int(chain[i + 1])) for i in range(10)]
    queries = small[:5] + q[:1] + small[5:] + q[1:]
    st = hold(ctx, k + 14, rows, cols, queries, max_hops=(-1, 1), slots=(64,))
    if role != "dst":
        assert st[(q[0][0], q[0][1], -1)][7] >= k


def test_three_fans_around_the_one_workgroup_sort(ctx):
    # three disjoint fans a -> leaves -> b in one graph: 2 * leaves pairs, below, at and above SD_SORT_MAX; ids descending
    rows, cols, queries, base = [], [], [], 0
    for leaves in (2047, 2048, 2049):
        b, a = base, base + leaves + 1
        mid = base + np.arange(leaves, 0, -1)
        rows += [np.full(leaves, a), mid]
        cols += [mid, np.full(leaves, b)]
        queries.append((a, b))
        base += leaves + 2
    assert 2 * 2048 == SD_SORT_MAX
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    queries = [(int(rows[0]), int(cols[0]))] + queries[:2] + [(int(cols[5]), 0)] + queries[2:]
    st = hold(ctx, base, rows, cols, queries, slots=(0, 2))
    assert [st[(s, d, -1)][7] for s, d in (queries[1], queries[2], queries[4])] == [2049, 2050, 2051]


def test_long_path_beside_a_one_hop_and_an_unreachable_query(ctx):
    n = 3000
    st = hold(ctx, n + 1, np.arange(n - 1), np.arange(1, n), [(0, n - 1), (10, 11), (5, n), (n - 1, 0)], slots=(0,))
    assert st[(0, n - 1, -1)][0] + st[(0, n - 1, -1)][1] == n - 1


@pytest.mark.parametrize("n", [65, 127])
def test_bitmap_tails_and_their_reset(ctx, n):
    # two routes of equal length between the first and the last vertex, through the highest ids
    rows, cols = [0, 0, n - 2, n - 3], [n - 2, n - 3, n - 1, n - 1]
    queries = [(0, n - 1), (n - 1, 0), (n - 1, n - 1), (0, n - 1), (0, n - 2), (0, n - 1), (n - 3, n - 1), (0, n - 1)]
    st = hold(ctx, n, rows, cols, queries, max_hops=(-1, 2, 1), slots=(3,))
    assert st[(0, n - 1, -1)][7] == 4


def test_hypersparse_input(ctx):
    n = 100_000
    rows, cols = np.array([7, 99_999, 50_000], dtype=U64), np.array([99_999, 50_000, 7], dtype=U64)
    order = np.argsort(rows)
    H = ctx.mat_from_csr(n, n, np.arange(4, dtype=U64), cols[order], hyper_rows=rows[order])
    hold(ctx, n, rows, cols, [(7, 50_000), (50_000, 50_000), (50_000, 99_999), (3, 7)], max_hops=(-1, 1), A=H)
    H.free()


def rmat_pairs(rng, deg_out, deg_in, k):
    """as tests/test_gpu_spdag.py builds them: the hub pairs, a hub cycle, hub targets"""
    top = np.argsort(deg_out + deg_in)[-2:]
    pairs = [(int(top[1]), int(top[0])), (int(top[0]), int(top[1])), (int(top[1]), int(top[1]))]
    live = np.nonzero((deg_out > 0) & (deg_in > 0))[0]
    while len(pairs) < k:
        s, d = rng.choice(live, 2)
        pairs.append((int(s), int(top[0]) if len(pairs) % 8 == 3 else int(d)))
    return pairs


@pytest.mark.parametrize("symmetric", [False, True])
def test_rmat_14_two_hundred_pairs(ctx, symmetric):
    R = ctx.mat_rmat(14)
    n = R.nrows
    rp, ci, _ = R.export_csr()
    rows, cols = np.repeat(np.arange(n), np.diff(rp.astype(np.int64))), ci.astype(np.int64)
    if symmetric:
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    A = ctx.mat_from_coo(n, n, rows.astype(U64), cols.astype(U64))
    R.free()
    pairs = rmat_pairs(np.random.default_rng(0xB7C), np.bincount(rows, minlength=n), np.bincount(cols, minlength=n), 200)
    st = hold(ctx, n, rows, cols, pairs, slots=(0, 7), sides=(0, 3), A=A, checked=32)
    A.free()
    assert any(s[0] and s[1] for s in st.values())   # both balls grew in some query


def test_two_batches_return_identical_arrays(ctx):
    A = ctx.mat_rmat(12)
    srcs, dsts = list(range(1, 41)), list(range(2, 42))
    a = engine.shortest_dag_batch(ctx, A, None, srcs, dsts, stats=True)
    b = engine.shortest_dag_batch(ctx, A, None, srcs, dsts, stats=True)
    A.free()
    for x, y in zip(a, b):
        assert x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:4], y[1:4])) and x[4] == y[4]
    assert any(x[0] > 0 for x in a)


def test_three_host_threads_batch_beside_single_calls(ctx):
    A = ctx.mat_rmat(12)
    At = A.transpose()
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows, cols = np.repeat(np.arange(n), np.diff(rp.astype(np.int64))), ci.astype(np.int64)
    prep = prepare(n, rows, cols)
    live = np.nonzero(np.diff(rp.astype(np.int64)))[0]
    errors = []

    def query(k, j):
        return int(live[(7 * k + 3 * j) % len(live)]), int(live[(11 * k + 5 * j + 1) % len(live)])

    def batches(k):
        try:
            for r in range(2):
                qs = [query(k, 12 * r + j) for j in range(12)]
                got = engine.shortest_dag_batch(ctx, A, At if r else None, [s for s, _ in qs], [d for _, d in qs])
                for q, g in zip(qs, got):
                    same_as_checker(g, shortest_dag(n, None, None, q[0], q[1], -1, prepared=prep), f"thread {k} batch {r} {q}")
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    def singles():
        try:
            for j in range(8):
                s, d = query(3, j)
                same_as_checker(engine.shortest_dag(ctx, A, At if j % 2 else None, s, d),
                                shortest_dag(n, None, None, s, d, -1, prepared=prep), f"single {j}")
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=batches, args=(k,)) for k in range(3)] + [threading.Thread(target=singles)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    At.free()
    A.free()
    assert not errors, errors


def test_arguments(ctx):
    A = ctx.mat_from_coo(4, 4, np.array([0, 1], dtype=U64), np.array([1, 2], dtype=U64))
    R = ctx.mat_from_coo(4, 5, np.array([0], dtype=U64), np.array([1], dtype=U64))
    assert engine.shortest_dag_batch(ctx, A, None, [], []) == []
    none = np.zeros(0, dtype=U64)
    for n in (1, 65):
        E = ctx.mat_from_coo(n, n, none, none)
        got = engine.shortest_dag_batch(ctx, E, None, [0, n - 1, 0], [n - 1, 0, 0], stats=True)
        assert [(g[0], len(g[1]), g[4]) for g in got] == [(-1, 0, [0] * 8)] * 3
        E.free()
    # an index out of range in the middle of a batch: refused before any work, the outputs untouched
    for srcs, dsts in (([0, 4, 1], [2, 0, 2]), ([0, 0, 1], [2, 2**40, 2])):
        with pytest.raises(FgpuError) as e:
            engine.shortest_dag_batch(ctx, A, None, srcs, dsts)
        assert e.value.code == FGPU_OUT_OF_BOUNDS and "query 1" in str(e.value)
    s, d = np.array([0, 4, 1], dtype=U64), np.array([2, 0, 2], dtype=U64)
    length, off, st = np.full(3, 77, dtype=np.int64), np.full(4, 77, dtype=U64), np.full(24, 77, dtype=U64)
    u64p = C.POINTER(C.c_uint64)
    f, t, dep = u64p(), u64p(), u64p()
    code = ctx.lib.fgpu_shortest_dag_batch(ctx._h, A._h, None, s.ctypes.data_as(u64p), d.ctypes.data_as(u64p), C.c_uint64(3),
                                           C.c_int64(-1), C.c_uint32(0), length.ctypes.data_as(C.POINTER(C.c_int64)),
                                           off.ctypes.data_as(u64p), C.byref(f), C.byref(t), C.byref(dep), st.ctypes.data_as(u64p))
    assert code == FGPU_OUT_OF_BOUNDS
    assert (length == 77).all() and (off == 77).all() and (st == 77).all() and not f and not t and not dep
    with pytest.raises(FgpuError):
        engine.shortest_dag_batch(ctx, R, None, [0], [1])
    with pytest.raises(FgpuError):
        engine.shortest_dag_batch(ctx, A, R, [0], [1])
    with pytest.raises(FgpuError) as e:
        engine.shortest_dag_batch(ctx, A, None, [0], [2], slots=65)
    assert e.value.code == FGPU_INVALID
    got = engine.shortest_dag_batch(ctx, A, None, [0], [2], slots=64)
    assert got[0][0] == 2 and got[0][1].tolist() == [0, 1] and got[0][2].tolist() == [1, 2] and got[0][3].tolist() == [0, 1]
    assert ctx.get_option("spdag_sides") == 0
    A.free()
    R.free()
