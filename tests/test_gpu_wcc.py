"""GPU: fgpu_wcc (algo.WCC's LAGr_ConnectedComponents core) against the numpy checker of tests/wcc_check.py.  The labels
are exact — component[v] = the smallest vertex id of v's component, -1 outside the active set — so every comparison is
array equality.  Every test runs under both forced wcc_mode values: Afforest with sampling and skip (1) and the full link
pass (2)."""
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wcc_check import components, csr_of, wcc_labels  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


@pytest.fixture(autouse=True, params=[1, 2], ids=["afforest", "full-pass"])
def mode(request, ctx):
    ctx.set_option("wcc_mode", request.param)
    yield request.param
    ctx.set_option("wcc_mode", 0)


def up(ctx, n, rows, cols):
    rp, ci = csr_of(n, rows, cols)
    A = ctx.mat_from_coo(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))
    return A, rp, ci


def sym(rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


def bitmap(act):
    """bool[n] -> the nrows-bit LSB-first u64 words fgpu_wcc takes"""
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


def run_both(ctx, n, rows, cols, active=None):
    """the directed entries with At, and the symmetrised pattern with At = None: both must give the checker's labels"""
    A, rp, ci = up(ctx, n, rows, cols)
    want = wcc_labels(n, rp, ci, active)
    At = A.transpose()
    act = bitmap(active) if active is not None else None
    got, st = engine.wcc(ctx, A, At, act, stats=True)
    assert np.array_equal(got, want)
    assert st[0] == components(want)
    sr, sc = sym(rows, cols)
    S = ctx.mat_from_coo(n, n, sr.astype(U64), sc.astype(U64))
    got2, st2 = engine.wcc(ctx, S, None, act, stats=True)
    assert np.array_equal(got2, want)
    assert st2[0] == st[0]
    return want


def test_empty_and_single_vertex(ctx):
    A = ctx.mat_new(0, 0)
    got, st = engine.wcc(ctx, A, None, stats=True)
    assert len(got) == 0 and st == [0, 0, 0, 0]
    one = ctx.mat_new(1, 1)
    got, st = engine.wcc(ctx, one, one.transpose(), stats=True)
    assert got.tolist() == [0] and st[0] == 1


def test_self_loops_duplicates_and_isolated_vertices(ctx):
    rows = [0, 0, 2, 2, 3, 5, 5, 5]
    cols = [0, 0, 2, 3, 2, 7, 7, 5]
    want = run_both(ctx, 9, rows, cols)
    assert want.tolist() == [0, 1, 2, 2, 4, 5, 6, 5, 8]


def test_path_star_and_trees_with_far_minima(ctx):
    n = 3000
    run_both(ctx, n, np.arange(n - 1), np.arange(1, n))                   # a path in id order
    run_both(ctx, n, np.arange(1, n)[::-1], np.arange(n - 1)[::-1])       # ... and reversed
    run_both(ctx, n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n))    # a star on vertex 0
    run_both(ctx, n, np.arange(1, n), np.full(n - 1, n - 1))              # a star on the LAST vertex
    # two trees: one whose minimum is a leaf at the deep end, one whose minimum is the root
    rng = np.random.default_rng(5)
    ids = rng.permutation(n)
    a, b = np.sort(ids[: n // 2])[::-1], ids[n // 2:]
    r1, c1 = a[1:], a[(np.arange(1, len(a)) - 1) // 2]                     # heap-shaped tree, root = max id, min = a leaf
    r2, c2 = b[1:], b[(np.arange(1, len(b)) - 1) // 2]
    want = run_both(ctx, n, np.concatenate([r1, r2]), np.concatenate([c1, c2]))
    assert components(want) == 2
    assert want[a[0]] == a.min() and want[b[0]] == b.min()


def test_directed_only_entries_join_through_the_transpose(ctx, mode):
    # every entry points from a larger id to a smaller one or the other way round; only A's direction is stored
    n = 200
    rows = np.arange(1, n)
    cols = np.arange(0, n - 1)
    A, rp, ci = up(ctx, n, cols, rows)                                     # i -> i + 1 only
    got, _ = engine.wcc(ctx, A, A.transpose())
    assert (got == 0).all()
    B, _, _ = up(ctx, n, rows, cols)                                       # i + 1 -> i only
    got, _ = engine.wcc(ctx, B, B.transpose())
    assert (got == 0).all()


def test_ids_near_the_end_of_a_large_id_space(ctx):
    n = (1 << 20) + 17
    rows = np.array([n - 1, n - 2, n - 3, 5, n - 1], dtype=np.int64)
    cols = np.array([n - 2, n - 3, 5, 7, n - 1], dtype=np.int64)
    want = run_both(ctx, n, rows, cols)
    assert want[n - 1] == 5 and want[7] == 5 and want[n - 4] == n - 4


@pytest.mark.parametrize("scale", [10, 13, 16])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rmat_matches_the_checker(ctx, scale, seed):
    A = ctx.mat_rmat(scale, 16, 0xC0C0 + 97 * seed + scale)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rp, ci = rp.astype(np.int64), ci.astype(np.int64)
    want = wcc_labels(n, rp, ci)
    got, st = engine.wcc(ctx, A, A.transpose(), stats=True)
    assert np.array_equal(got, want)
    assert st[0] == components(want)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    sr, sc = sym(rows, ci)
    S = ctx.mat_from_coo(n, n, sr.astype(U64), sc.astype(U64))
    got2, st2 = engine.wcc(ctx, S, None, stats=True)
    assert np.array_equal(got2, want) and st2[0] == st[0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_active_bitmap_induced_subgraph(ctx, seed):
    rng = np.random.default_rng(seed)
    A = ctx.mat_rmat(12, 8, 0xAC7 + seed)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    act = rng.random(n) < (0.3, 0.6, 0.9)[seed]
    run_both(ctx, n, rows, ci.astype(np.int64), act)
    # a path through an inactive vertex does not join its ends
    act = np.ones(10, dtype=bool)
    act[4] = False
    got = run_both(ctx, 10, np.arange(9), np.arange(1, 10), act)
    assert got.tolist() == [0, 0, 0, 0, -1, 5, 5, 5, 5, 5]


def test_hypersparse_inputs_give_the_labels_of_the_dense_rows(ctx):
    """A and / or A' stored hypersparse (row list + short row pointers) are densified for the call: identical labels and
    component counts, with a transpose and (symmetric pattern) without, with and without an active bitmap."""
    n = 6000
    rng = np.random.default_rng(41)
    some = rng.choice(n, 400, replace=False)                            # most rows and columns are empty
    rows, cols = rng.choice(some, 1500), rng.choice(some, 1500)
    A, rp, ci = up(ctx, n, rows, cols)
    At = A.transpose()
    hA, hAt = hypersparse(ctx, A), hypersparse(ctx, At)
    sr, sc = sym(rows, cols)
    S = ctx.mat_from_coo(n, n, sr.astype(U64), sc.astype(U64))
    hS = hypersparse(ctx, S)
    for act in (None, bitmap(rng.random(n) < 0.7)):
        want, st = engine.wcc(ctx, A, At, act, stats=True)
        for A_, At_ in ((hA, hAt), (hA, At), (A, hAt)):
            got, st_ = engine.wcc(ctx, A_, At_, act, stats=True)
            assert np.array_equal(got, want) and st_[0] == st[0]           # (entries read depend on the order of the hooks)
        want2, st2 = engine.wcc(ctx, S, None, act, stats=True)
        got2, st2_ = engine.wcc(ctx, hS, None, act, stats=True)
        assert np.array_equal(got2, want2) and st2_[0] == st2[0] and np.array_equal(want2, want)
    assert np.array_equal(engine.wcc(ctx, hA, hAt)[0], wcc_labels(n, rp, ci))


def test_bits_past_n_in_the_active_bitmap_are_not_vertices(ctx):
    """n is not a multiple of 64: the last word's bits at and past n are ignored (the sample and the link kernels test
    neighbours' bits, never one past n) — labels and component count are those of the clean bitmap."""
    n = 5000 - 23
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    A, rp, ci = up(ctx, n, rows, cols)
    At = A.transpose()
    active = rng.random(n) < 0.6
    clean = bitmap(active)
    dirty = clean.copy()
    dirty[-1] |= U64(~((1 << (n % 64)) - 1) & 0xFFFFFFFFFFFFFFFF)
    assert n % 64 and dirty[-1] != clean[-1]
    want, st = engine.wcc(ctx, A, At, clean, stats=True)
    got, st_ = engine.wcc(ctx, A, At, dirty, stats=True)
    assert np.array_equal(got, want) and st_[0] == st[0]                   # (entries read depend on the order of the hooks)
    assert np.array_equal(got, wcc_labels(n, rp, ci, active))


_RMAT22 = {}


def test_rmat22_exact_and_the_skip_runs(ctx, mode, bench_graphs):
    A, At, a = bench_graphs(22)
    n = a.nrows
    if "want" not in _RMAT22:   # (the checker's labels, once for both modes)
        _RMAT22["want"] = wcc_labels(n, a.rowptr.astype(np.int64), a.colidx.astype(np.int64))
    want = _RMAT22["want"]
    got, st = engine.wcc(ctx, A, At, stats=True)
    assert np.array_equal(got, want)
    assert st[0] == components(want)
    if mode == 2:
        assert st[1] == A.nvals and st[3] == 0
    else:
        assert st[1] < A.nvals                       # the giant component's rows were skipped
        giant = np.bincount(want[want >= 0]).max()
        assert st[3] == giant


def test_pinned_and_pageable_outputs_agree(ctx):
    A = ctx.mat_rmat(15, 16, 0x9199)
    At = A.transpose()
    n = A.nrows
    pinned = ctx.host_array(n, np.int64)
    a, _ = engine.wcc(ctx, A, At, out=pinned)
    b, _ = engine.wcc(ctx, A, At)
    c, _ = engine.wcc(ctx, A, At)
    assert a is pinned
    assert np.array_equal(a, b) and np.array_equal(b, c)


def test_three_threads_on_one_context(ctx):
    graphs = []
    for k in range(3):
        A = ctx.mat_rmat(12 + k, 16, 0x7A + k)
        rp, ci, _ = A.export_csr()
        graphs.append((A, A.transpose(), wcc_labels(A.nrows, rp.astype(np.int64), ci.astype(np.int64))))
    errors, results = [], [None] * 3

    def work(k):
        try:
            A, At, _ = graphs[k]
            for _ in range(4):
                got, _ = engine.wcc(ctx, A, At)
                results[k] = got
                assert np.array_equal(got, graphs[k][2])
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(3):
        assert np.array_equal(results[k], graphs[k][2])


def test_error_codes(ctx):
    A = ctx.mat_rmat(8, 4, 3)
    rect = ctx.mat_new(4, 5)
    other = ctx.mat_new(A.nrows + 1, A.nrows + 1)
    before = ctx.device_bytes()
    with pytest.raises(FgpuError) as e:
        engine.wcc(ctx, rect)
    assert e.value.code == -6                                          # FGPU_DIM_MISMATCH
    with pytest.raises(FgpuError) as e:
        engine.wcc(ctx, A, other)
    assert e.value.code == -6
    out = np.zeros(A.nrows, dtype=np.int64)
    st = np.zeros(4, dtype=U64)
    code = ctx.lib.fgpu_wcc(ctx._h, A._h, None, None, None, st.ctypes.data_as(engine.u64p))
    assert code == -2                                                  # FGPU_NULL_POINTER
    assert ctx.device_bytes() == before
    engine.wcc(ctx, A, None, out=out)                                  # the context still works
    with pytest.raises(FgpuError):
        ctx.set_option("wcc_mode", 3)
    assert ctx.get_option("wcc_mode") in (1, 2)
