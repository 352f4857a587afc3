"""GPU: fgpu_betweenness (algo.betweenness' LAGr_Betweenness core) against the numpy checker of tests/bc_check.py, every case at
|got - ref| <= 1e-9 * max(1, |ref|).  bc_direction 1 (push), 2 (pull) and 0 (auto) must agree bit for bit, and so must
repeated calls; batch widths agree within the tolerance."""
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bc_check import betweenness, csr_of  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


@pytest.fixture(autouse=True)
def reset_options(ctx):
    yield
    ctx.set_option("bc_batch", 0)
    ctx.set_option("bc_direction", 0)


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.abs(got - want) > 1e-9 * np.maximum(1.0, np.abs(want))
    assert not bad.any(), (np.flatnonzero(bad)[:10], got[bad][:10], want[bad][:10])


def up(ctx, n, rows, cols):
    A = ctx.mat_from_coo(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))
    rp, ci = csr_of(n, rows, cols)
    return A, rp, ci


def bitmap(act):
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


def run_dirs(ctx, A, At, sources, act=None):
    """the three directions: bit-identical; returns (centrality, stats of the auto run)"""
    out = {}
    for d in (1, 2, 0):
        ctx.set_option("bc_direction", d)
        out[d] = engine.betweenness(ctx, A, sources, At, act, stats=True)
    ctx.set_option("bc_direction", 0)
    assert np.array_equal(out[1][0], out[2][0]) and np.array_equal(out[0][0], out[1][0])
    assert out[1][1][3] == out[2][1][3] == out[0][1][3]     # deepest level
    return out[0]


def test_empty_and_one_vertex(ctx):
    A = ctx.mat_new(0, 0)
    got, st = engine.betweenness(ctx, A, [], stats=True)
    assert len(got) == 0 and st == [0, 0, 0, 0]
    one = ctx.mat_new(1, 1)
    got, st = engine.betweenness(ctx, one, [0, 0], stats=True)
    assert got.tolist() == [0.0] and st[0] == 1 and st[3] == 0
    got, st = engine.betweenness(ctx, one, [], stats=True)
    assert got.tolist() == [0.0] and st == [0, 0, 0, 0]


def test_hand_graphs_sources_that_reach_nothing_and_duplicates(ctx):
    A, rp, ci = up(ctx, 5, [0, 1, 1, 2, 3], [1, 2, 3, 4, 4])
    got, st = run_dirs(ctx, A, A.transpose(), np.arange(5))
    assert got.tolist() == [0, 3, 1, 1, 0] and st[3] == 3
    got, _ = run_dirs(ctx, A, None, [4, 4, 4])                   # E has no out-edges
    assert got.tolist() == [0] * 5
    got, _ = run_dirs(ctx, A, None, [0, 0, 1])                   # a duplicate counts twice
    close(got, betweenness(5, rp, ci, [0, 0, 1])[0])
    B, rp, ci = up(ctx, 6, [0, 0, 0, 1, 2, 3, 3, 3, 5], [0, 1, 2, 3, 3, 4, 3, 4, 5])   # diamond, self-loops, repeats
    got, _ = run_dirs(ctx, B, B.transpose(), [0, 5, 3])
    close(got, betweenness(6, rp, ci, [0, 5, 3])[0])
    assert got.tolist() == [0, 1, 1, 1, 0, 0]


def test_path_deeper_than_a_byte(ctx):
    n = 2000
    A, rp, ci = up(ctx, n, np.arange(n - 1), np.arange(1, n))
    src = [0, 1, 700, 1998]
    got, st = run_dirs(ctx, A, A.transpose(), src)
    close(got, betweenness(n, rp, ci, src)[0])
    assert st[3] == n - 1


def test_hub_rows(ctx):
    # vertex 0 -> 9000 leaves, each leaf -> 1 -> 2: the rows of 0 (out) and of 1 (in) are hub rows in A and A'
    n = 9003
    leaves = np.arange(3, n)
    rows = np.concatenate([np.zeros(len(leaves), dtype=np.int64), leaves, [1, 2]])
    cols = np.concatenate([leaves, np.ones(len(leaves), dtype=np.int64), [2, 0]])
    A, rp, ci = up(ctx, n, rows, cols)
    src = [0, 1, 2, 3, 4000]
    got, _ = run_dirs(ctx, A, A.transpose(), src)
    close(got, betweenness(n, rp, ci, src)[0])


@pytest.mark.parametrize("nsrc", [1, 15, 16, 63, 64, 65, 130])
def test_source_counts_and_batch_widths(ctx, nsrc):
    A = ctx.mat_rmat(12, 8, 0xBC00 + nsrc)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rng = np.random.default_rng(nsrc)
    src = rng.integers(0, n, nsrc)
    want = betweenness(n, rp.astype(np.int64), ci.astype(np.int64), src)[0]
    At = A.transpose()
    for width in (0, 1, 7, 16, 64):
        ctx.set_option("bc_batch", width)
        got, st = engine.betweenness(ctx, A, src, At, stats=True)
        close(got, want)
        if width:
            assert st[0] == -(-nsrc // width)


@pytest.mark.parametrize("scale", [12, 14, 16])
def test_rmat_directions_and_repeats(ctx, scale):
    A = ctx.mat_rmat(scale, 16, 0xB7 + scale)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    At = A.transpose()
    src = np.concatenate([np.arange(8), np.random.default_rng(scale).integers(0, n, 24)])
    want, deepest = betweenness(n, rp.astype(np.int64), ci.astype(np.int64), src)
    got, st = run_dirs(ctx, A, At, src)
    close(got, want)
    assert st[3] == deepest and st[0] == 1
    again, _ = engine.betweenness(ctx, A, src, At)
    assert np.array_equal(again, got)
    nat, _ = engine.betweenness(ctx, A, src)                   # the cached transpose
    assert np.array_equal(nat, got)


@pytest.mark.parametrize("seed", [0, 1])
def test_active_bitmap_induced_subgraph(ctx, seed):
    A = ctx.mat_rmat(12, 8, 0xAC7 + seed)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rng = np.random.default_rng(seed)
    act = rng.random(n) < (0.5, 0.9)[seed]
    src = rng.choice(np.flatnonzero(act), 20, replace=False)
    want = betweenness(n, rp.astype(np.int64), ci.astype(np.int64), src, act)[0]
    got, _ = run_dirs(ctx, A, A.transpose(), src, bitmap(act))
    close(got, want)
    assert (got[~act] == 0).all()


def test_hypersparse_inputs_give_the_bits_of_the_dense_rows(ctx):
    """A and / or A' stored hypersparse (row list + short row pointers) are densified for the call: identical scores and
    counters in every direction, with the caller's transpose and with the cached one, with and without an active bitmap —
    and the one-shot fgpu_bfs, which shares that prelude, returns identical levels, parents and edge counts."""
    n = 6000
    rng = np.random.default_rng(43)
    some = rng.choice(n, 400, replace=False)                            # most rows and columns are empty
    rows = np.concatenate([rng.choice(some, 3000), np.full(4500, some[0])])
    cols = np.concatenate([rng.choice(some, 3000), rng.choice(n, 4500, replace=False)])   # + a hub row of 4500 out-edges
    A, rp, ci = up(ctx, n, rows, cols)
    At = A.transpose()
    hA, hAt = hypersparse(ctx, A), hypersparse(ctx, At)
    src = np.concatenate([some[:20], [some[0]]])
    for act in (None, bitmap(np.isin(np.arange(n), some) | (rng.random(n) < 0.5))):
        want, st = run_dirs(ctx, A, At, src, act)
        for A_, At_ in ((hA, hAt), (hA, At), (A, hAt), (hA, None)):
            got, st_ = run_dirs(ctx, A_, At_, src, act)
            assert np.array_equal(got, want) and st_ == st
    close(run_dirs(ctx, hA, hAt, src)[0], betweenness(n, rp, ci, src)[0])
    for s in (int(some[0]), int(some[7])):
        want = engine.bfs(ctx, A, At, s, -1, want_parent=True)
        for A_, At_ in ((hA, hAt), (hA, At), (A, hAt), (hA, None)):
            got = engine.bfs(ctx, A_, At_, s, -1, want_parent=True)
            assert np.array_equal(got[0], want[0]) and got[2] == want[2]
            assert ((got[0] >= 0) == (got[1] >= 0)).all()               # (which parent wins a level is the kernels' choice)
            reached = np.flatnonzero((got[0] > 0))
            assert (want[0][got[1][reached]] == got[0][reached] - 1).all()
        assert (want[0] >= 0).sum() > 1


def test_bits_past_n_in_the_active_bitmap_are_not_vertices(ctx):
    """n is not a multiple of 64: the last word's bits at and past n are ignored — scores and counters are those of the clean
    bitmap in every direction."""
    n = 5000 - 23
    rng = np.random.default_rng(9)
    rows, cols = rng.integers(0, n, 12000), rng.integers(0, n, 12000)
    A, rp, ci = up(ctx, n, rows, cols)
    At = A.transpose()
    active = rng.random(n) < 0.7
    clean = bitmap(active)
    dirty = clean.copy()
    dirty[-1] |= U64(~((1 << (n % 64)) - 1) & 0xFFFFFFFFFFFFFFFF)
    assert n % 64 and dirty[-1] != clean[-1]
    src = np.flatnonzero(active)[-20:]                                   # (the last word's vertices among them)
    want, st = run_dirs(ctx, A, At, src, clean)
    got, st_ = run_dirs(ctx, A, At, src, dirty)
    assert np.array_equal(got, want) and st_ == st
    close(got, betweenness(n, rp, ci, src, active)[0])


def test_rmat22_sixteen_sources(ctx, bench_graphs):
    A, At, a = bench_graphs(22)
    src = np.arange(16)
    want, deepest = betweenness(a.nrows, a.rowptr.astype(np.int64), a.colidx.astype(np.int64), src)
    got, st = run_dirs(ctx, A, At, src)
    close(got, want)
    assert st[3] == deepest and st[0] == 1


def test_pinned_and_pageable_outputs_agree(ctx):
    A = ctx.mat_rmat(15, 16, 0x9199)
    At = A.transpose()
    src = np.arange(0, A.nrows, 997)
    pinned = ctx.host_array(A.nrows, np.float64)
    a, _ = engine.betweenness(ctx, A, src, At, out=pinned)
    b, _ = engine.betweenness(ctx, A, src, At)
    assert a is pinned
    assert np.array_equal(a, b)


def test_three_threads_on_one_context(ctx):
    graphs = []
    for k in range(3):
        A = ctx.mat_rmat(11 + k, 16, 0x7B + k)
        rp, ci, _ = A.export_csr()
        src = np.arange(0, A.nrows, 61 + k)
        graphs.append((A, A.transpose(), src, betweenness(A.nrows, rp.astype(np.int64), ci.astype(np.int64), src)[0]))
    errors, results = [], [None] * 3

    def work(k):
        try:
            A, At, src, want = graphs[k]
            for _ in range(3):
                got, _ = engine.betweenness(ctx, A, src, At)
                if results[k] is not None:
                    assert np.array_equal(got, results[k])
                results[k] = got
                close(got, want)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_error_codes(ctx):
    A = ctx.mat_rmat(8, 4, 3)
    n = A.nrows
    rect = ctx.mat_new(4, 5)
    other = ctx.mat_new(n + 1, n + 1)
    before = ctx.device_bytes()
    with pytest.raises(FgpuError) as e:
        engine.betweenness(ctx, rect, [0])
    assert e.value.code == -6                                          # FGPU_DIM_MISMATCH
    with pytest.raises(FgpuError) as e:
        engine.betweenness(ctx, A, [0], other)
    assert e.value.code == -6
    with pytest.raises(FgpuError) as e:
        engine.betweenness(ctx, A, [0, n])
    assert e.value.code == -105                                        # FGPU_OUT_OF_BOUNDS
    act = np.zeros(n, dtype=bool)
    act[:10] = True
    with pytest.raises(FgpuError) as e:
        engine.betweenness(ctx, A, [3, 20], None, bitmap(act))
    assert e.value.code == -3                                          # FGPU_INVALID
    out = np.zeros(n, dtype=np.float64)
    src = np.zeros(1, dtype=U64)
    lib, P = ctx.lib, engine.u64p
    dp = engine.C.POINTER(engine.C.c_double)
    assert lib.fgpu_betweenness(ctx._h, None, None, None, src.ctypes.data_as(P), 1, out.ctypes.data_as(dp), None) == -2
    assert lib.fgpu_betweenness(ctx._h, A._h, None, None, src.ctypes.data_as(P), 1, None, None) == -2
    assert lib.fgpu_betweenness(ctx._h, A._h, None, None, None, 1, out.ctypes.data_as(dp), None) == -2
    assert ctx.device_bytes() == before
    out[:] = 1.0
    assert lib.fgpu_betweenness(ctx._h, A._h, None, None, None, 0, out.ctypes.data_as(dp), None) == 0
    assert (out == 0).all()                                            # no sources: all zeros
    for name, bad in (("bc_batch", 65), ("bc_batch", -1), ("bc_direction", 3)):
        with pytest.raises(FgpuError):
            ctx.set_option(name, bad)
    ctx.set_option("bc_batch", 32)
    ctx.set_option("bc_direction", 2)
    assert ctx.get_option("bc_batch") == 32 and ctx.get_option("bc_direction") == 2
    engine.betweenness(ctx, A, [0, 1], out=out)                        # the context still works
