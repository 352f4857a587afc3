"""GPU: fgpu_cdlp (algo.labelPropagation's LAGraph_cdlp core) against the numpy checker of tests/cdlp_check.py.  The algorithm
is deterministic — synchronous iterations, ties to the smallest label — so every comparison is array equality, the four
stats counters included."""
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdlp_check import cdlp_stats, csr_of  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


def sym(rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


def up(ctx, n, rows, cols):
    rp, ci = csr_of(n, rows, cols)
    S = ctx.mat_from_coo(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))
    return S, rp, ci


def bitmap(act):
    """bool[n] -> the nrows-bit LSB-first u64 words fgpu_cdlp takes"""
    n = len(act)
    bits = np.zeros((n + 63) // 64 * 64, dtype=bool)
    bits[:n] = act
    return np.packbits(bits, bitorder="little").view(np.uint64)


def hypersparse(ctx, m):
    """The same entries stored as a delta layer stores them: the ids of the non-empty rows + a row-pointer array over those."""
    rp, ci, _ = m.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(m.nrows, m.ncols, short, ci, hyper_rows=rows)


def check(ctx, S, n, rp, ci, itermax, active=None):
    want, wst = cdlp_stats(n, rp, ci, itermax, active)
    got, st = engine.cdlp(ctx, S, bitmap(active) if active is not None else None, itermax, stats=True)
    assert np.array_equal(got, want), (itermax, np.flatnonzero(got != want)[:10])
    assert st == wst, (itermax, st, wst)
    return want, wst


def run(ctx, n, rows, cols, itermax, active=None):
    S, rp, ci = up(ctx, n, rows, cols)
    return check(ctx, S, n, rp, ci, itermax, active)


def test_empty_and_single_vertex(ctx):
    S = ctx.mat_new(0, 0)
    got, st = engine.cdlp(ctx, S, stats=True)
    assert len(got) == 0 and st == [0, 0, 0, 0]
    one = ctx.mat_new(1, 1)
    got, st = engine.cdlp(ctx, one, stats=True)
    assert got.tolist() == [0] and st == [1, 0, 0, 1]
    loop = ctx.mat_from_coo(1, 1, np.array([0], dtype=U64), np.array([0], dtype=U64))
    got, st = engine.cdlp(ctx, loop, itermax=7, stats=True)
    assert got.tolist() == [0] and st == [1, 0, 1, 1]


def test_hand_cases(ctx):
    # a tie goes to the smaller label
    rows, cols = sym([4, 4, 4, 5, 5], [3, 1, 2, 3, 2])
    want, _ = run(ctx, 6, rows, cols, 1)
    assert want[4] == 1 and want[5] == 2
    # frequency first: two votes for 7 beat one for 0
    want, _ = run(ctx, 9, [6, 8, 8, 8, 7], [7, 0, 7, 6, 7], 2)
    assert want[6] == 7 and want[8] == 7
    # a 2-path oscillates with period 2
    rows, cols = sym([0], [1])
    assert run(ctx, 2, rows, cols, 3)[0].tolist() == [1, 0]
    assert run(ctx, 2, rows, cols, 4)[0].tolist() == [0, 1]
    # a self-loop votes; an isolated vertex keeps its id
    rows, cols = sym([2], [3])
    assert run(ctx, 5, rows, cols, 1)[0].tolist() == [0, 1, 3, 2, 4]
    assert run(ctx, 5, np.append(rows, 2), np.append(cols, 2), 1)[0].tolist() == [0, 1, 2, 2, 4]
    # itermax = 0 is the identity, with and without a bitmap
    want, st = run(ctx, 5, rows, cols, 0)
    assert want.tolist() == [0, 1, 2, 3, 4] and st == [0, 0, 0, 5]
    want, st = run(ctx, 5, rows, cols, 0, np.array([True, False, True, True, False]))
    assert want.tolist() == [0, -1, 2, 3, -1] and st == [0, 0, 0, 3]


def test_duplicate_pairs_are_one_entry_and_one_vote(ctx):
    # vertex 2: the loop given three times and the neighbour 3 once — a tie of one vote each, which keeps 2
    rows = [2, 2, 2, 2, 3, 3]
    cols = [2, 2, 2, 3, 2, 2]
    want, st = run(ctx, 4, rows, cols, 1)
    assert want.tolist() == [0, 1, 2, 2]
    assert st[2] == 3                                                       # three stored entries, read once


def test_early_convergence_stops_the_run(ctx):
    # disjoint triangles settle on their smallest vertex in two iterations; the third changes nothing and ends the run
    k = 500
    base = 3 * np.arange(k)
    rows, cols = sym(np.concatenate([base, base + 1, base + 2]), np.concatenate([base + 1, base + 2, base]))
    for itermax in (10, 100, 3, 4, 5):
        want, st = run(ctx, 3 * k, rows, cols, itermax)
        assert st[0] == 3 and st[0] <= itermax and st[1] == 0
        assert np.array_equal(want, np.repeat(base, 3))
        assert st[3] == k
    want, st = run(ctx, 3 * k, rows, cols, 2)                               # the labels are there already, unconfirmed
    assert st[0] == 2 and st[1] > 0 and np.array_equal(want, np.repeat(base, 3))


def planted(n):
    """Stars and cliques with rows of exactly 1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 20 000 and 70 000 stored entries.
    -> (rows, cols, the centre whose 69 999 leaves all end with its label, the centre whose 20 000 neighbours keep their own)"""
    nxt = [0]

    def take(k):
        a = np.arange(nxt[0], nxt[0] + k, dtype=np.int64)
        nxt[0] += k
        return a

    R, C = [], []

    def edges(a, b):
        R.extend([a, b])
        C.extend([b, a])

    # a centre with a self-loop and a smaller id than its 69 999 leaves: everything takes the centre's label and stays
    one = take(1)
    leaves = take(69999)
    edges(np.repeat(one, len(leaves)), leaves)
    R.append(one)
    C.append(one)
    # 20 000 neighbours u, each with a self-loop and a pendant p (itself with a self-loop): u keeps its own label for ever
    # (two votes against the centre's one), so the centre always meets 20 000 distinct labels
    u, p = take(20000), take(20000)
    many = take(1)
    edges(u, p)
    edges(np.repeat(many, len(u)), u)
    R.extend([u, p])
    C.extend([u, p])
    # plain stars: centre and leaves swap labels every iteration
    for d in (1, 2, 3, 63, 64, 65, 4095, 4096, 4097):
        c = take(1)
        lv = take(d)
        edges(np.repeat(c, d), lv)
    # cliques: rows of 39 (short) and 65 (mid) entries, and of 40 / 66 with the self-loops of the second pair
    for size, loops in ((40, False), (66, False), (40, True), (66, True)):
        q = take(size)
        a, b = np.meshgrid(q, q)
        keep = (a != b) | loops
        R.append(a[keep])
        C.append(b[keep])
    assert nxt[0] <= n
    return np.concatenate(R), np.concatenate(C), int(one[0]), int(many[0])


def test_rows_of_every_class_and_their_boundaries(ctx):
    n = (1 << 17) - 29                                                      # not a multiple of 64
    rows, cols, one, many = planted(n)
    S, rp, ci = up(ctx, n, rows, cols)
    deg = set(np.diff(rp).tolist())
    assert {0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 20000, 70000} <= deg
    for itermax in (1, 2, 5):
        want, st = check(ctx, S, n, rp, ci, itermax)
    assert st[0] == 5 and st[1] > 0                                         # the plain stars never settle
    assert (want[ci[rp[one]:rp[one + 1]]] == one).all()                     # a hub whose neighbours all carry one label
    assert len(np.unique(want[ci[rp[many]:rp[many + 1]]])) == 20000         # a hub whose neighbours all differ
    # inactive hubs and inactive leaves: the hub rows are skipped, their votes are not cast
    rng = np.random.default_rng(3)
    act = rng.random(n) < 0.7
    act[one] = False
    for itermax in (1, 4):
        check(ctx, S, n, rp, ci, itermax, act)
    act = rng.random(n) < 0.5
    act[[one, many]] = [True, False]
    check(ctx, S, n, rp, ci, 3, act)


@pytest.mark.parametrize("itermax", [1, 2, 10])
def test_random_symmetric_graphs(ctx, itermax):
    n = 1 << 16
    for seed, per in ((1, 2), (2, 8), (3, 24)):
        rng = np.random.default_rng(100 * itermax + seed)
        m = per * n
        rows, cols = sym(rng.integers(0, n, m), rng.integers(0, n, m))
        run(ctx, n, rows, cols, itermax)


def test_symmetrised_rmat16(ctx):
    A = ctx.mat_rmat(16, 16, 0xCD17)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    sr, sc = sym(rows, ci.astype(np.int64))
    S, rp, ci = up(ctx, n, sr, sc)
    assert np.diff(rp).max() >= 4096                                        # hub rows are part of it
    want, st = check(ctx, S, n, rp, ci, 10)
    assert st[0] >= 2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_active_bitmap_induced_subgraph(ctx, seed):
    rng = np.random.default_rng(seed)
    n = 5000 - 23                                                           # the last bitmap word is partial
    m = 30000
    rows, cols = sym(rng.integers(0, n, m), rng.integers(0, n, m))
    S, rp, ci = up(ctx, n, rows, cols)
    active = rng.random(n) < (0.3, 0.6, 0.9)[seed]
    for itermax in (1, 3, 10):
        want, st = check(ctx, S, n, rp, ci, itermax, active)
    # bits at and past n in the last word are not vertices
    clean = bitmap(active)
    dirty = clean.copy()
    dirty[-1] |= U64(~((1 << (n % 64)) - 1) & 0xFFFFFFFFFFFFFFFF)
    assert dirty[-1] != clean[-1]
    got, gst = engine.cdlp(ctx, S, dirty, 10, stats=True)
    assert np.array_equal(got, want) and gst == st
    # a path through an inactive vertex: its two sides never exchange labels
    act = np.ones(7, dtype=bool)
    act[3] = False
    r, c = sym(np.arange(6), np.arange(1, 7))
    want, _ = run(ctx, 7, r, c, 6, act)
    assert want[3] == -1 and set(want[:3].tolist()) <= {0, 1, 2} and set(want[4:].tolist()) <= {4, 5, 6}


def test_hypersparse_input_gives_the_labels_of_the_dense_rows(ctx):
    n = 6000
    rng = np.random.default_rng(41)
    some = rng.choice(n, 400, replace=False)                               # most rows and columns are empty
    rows, cols = sym(rng.choice(some, 1500), rng.choice(some, 1500))
    S, rp, ci = up(ctx, n, rows, cols)
    hS = hypersparse(ctx, S)
    for active in (None, rng.random(n) < 0.7):
        for itermax in (1, 10):
            check(ctx, S, n, rp, ci, itermax, active)
            check(ctx, hS, n, rp, ci, itermax, active)


def test_pinned_and_pageable_outputs_agree(ctx):
    A = ctx.mat_rmat(14, 8, 0x9199)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    sr, sc = sym(rows, ci.astype(np.int64))
    S = ctx.mat_from_coo(n, n, sr.astype(U64), sc.astype(U64))
    pinned = ctx.host_array(n, np.int64)
    a, _ = engine.cdlp(ctx, S, out=pinned)
    b, _ = engine.cdlp(ctx, S)
    c, _ = engine.cdlp(ctx, S)
    assert a is pinned
    assert np.array_equal(a, b) and np.array_equal(b, c)


def test_two_threads_on_the_same_matrix(ctx):
    rng = np.random.default_rng(77)
    n = 1 << 14
    rows, cols = sym(rng.integers(0, n, 6 * n), rng.integers(0, n, 6 * n))
    star = np.arange(1, 6000)                                                # a hub row, so that both threads use the hub scratch
    rows, cols = np.concatenate([rows, np.zeros(len(star), dtype=np.int64), star]), np.concatenate([cols, star, np.zeros(len(star), dtype=np.int64)])
    S, rp, ci = up(ctx, n, rows, cols)
    want = {k: cdlp_stats(n, rp, ci, k) for k in (3, 10)}
    errors = []

    def work(k):
        try:
            for _ in range(4):
                got, st = engine.cdlp(ctx, S, None, k, stats=True)
                assert np.array_equal(got, want[k][0]) and st == want[k][1]
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in (3, 10)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_error_codes(ctx):
    A = ctx.mat_rmat(8, 4, 3)
    rect = ctx.mat_new(4, 5)
    before = ctx.device_bytes()
    with pytest.raises(FgpuError) as e:
        engine.cdlp(ctx, rect)
    assert e.value.code == -6                                          # FGPU_DIM_MISMATCH
    with pytest.raises(FgpuError) as e:
        engine.cdlp(ctx, A, itermax=-1)
    assert e.value.code == -3                                          # FGPU_INVALID
    out = np.zeros(A.nrows, dtype=np.int64)
    st = np.zeros(4, dtype=U64)
    code = ctx.lib.fgpu_cdlp(ctx._h, A._h, None, 10, None, st.ctypes.data_as(engine.u64p))
    assert code == -2                                                  # FGPU_NULL_POINTER
    code = ctx.lib.fgpu_cdlp(ctx._h, None, None, 10, out.ctypes.data_as(engine.i64p), None)
    assert code == -2
    code = ctx.lib.fgpu_cdlp(None, A._h, None, 10, out.ctypes.data_as(engine.i64p), None)
    assert code == -2
    assert ctx.device_bytes() == before
    engine.cdlp(ctx, A, out=out)                                       # the context still works
