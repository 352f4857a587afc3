"""GPU: fgpu_sssp (algo.SPpaths' single-source core) against the Dijkstra + tight-entry checker of tests/sssp_check.py.  The
distance of a vertex is unique and the parent is a pure function of the distances, so every comparison is array equality: dist
as BIT PATTERNS, parent and the deepest depth exactly."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of  # noqa: E402
from sssp_check import sssp  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
HUB_DEG = 4096   # common.hpp
AUTO = 4096      # "sssp_delta_log2": the derived width


def upload(ctx, n, rows, cols, bits):
    rows, cols = np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64)
    return ctx.mat_from_coo(n, n, rows, cols, None if bits is None else np.asarray(bits, dtype=U64))


def same(got, want):
    dist, parent, st = got
    wd, wp, wdepth = want
    assert np.array_equal(dist.view(U64), wd.view(U64)), "dist differs from the checker's bits"
    assert np.array_equal(parent, wp), "parent differs"
    assert st[3] == int(wdepth.max()), "deepest depth differs"


def check(ctx, n, rows, cols, bits, src, W=None):
    """run fgpu_sssp and compare everything with the checker; returns (stats, (dist, parent))"""
    own = W is None
    if own:
        W = upload(ctx, n, rows, cols, bits)
    want = sssp(n, rows, cols, bits, src)
    got = engine.sssp(ctx, W, src, stats=True)
    same(got, want)
    # without the parent search: the same distances
    d2, p2 = engine.sssp(ctx, W, src, want_parent=False)
    assert p2 is None and np.array_equal(d2.view(U64), want[0].view(U64))
    if own:
        W.free()
    return got[2], got


def random_pairs(rng, n, m, lo=0):
    """m distinct ordered pairs (a != b) with both ends in [lo, n)"""
    a = rng.integers(lo, n, 2 * m + 8)
    b = rng.integers(lo, n, 2 * m + 8)
    key = np.unique((a.astype(np.int64) * n + b)[a != b])
    key = rng.permutation(key)[:m]
    assert len(key) == m
    return key // n, key % n


def hashed(rows, cols, kind):
    """weights that are a fixed hash of (row, col): integers 1 .. 100, or uniform doubles in [0, 1)"""
    z = (np.asarray(rows, dtype=U64) << U64(32)) ^ np.asarray(cols, dtype=U64)
    z = (z + U64(0x9E3779B97F4A7C15)) * U64(0xBF58476D1CE4E5B9)
    z ^= z >> U64(29)
    z *= U64(0x94D049BB133111EB)
    z ^= z >> U64(32)
    if kind == "int":
        return (z % U64(100) + U64(1)).astype(np.float64)
    return (z >> U64(11)).astype(np.float64) / float(1 << 53)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_degenerate_sizes(ctx, n):
    none = np.zeros(0, dtype=np.int64)
    st, (dist, parent, _) = check(ctx, n, none, none, bits_of([]), 0)
    assert dist[0] == 0.0 and parent[0] == 0 and np.isinf(dist[1:]).all() and (parent[1:] == -1).all()
    check(ctx, n, none, none, None, n - 1)
    if n > 1:
        st, (dist, parent, _) = check(ctx, n, [0], [n - 1], bits_of([2.5]), 0)
        assert dist[n - 1] == 2.5 and parent[n - 1] == 0 and st[3] == 1
        check(ctx, n, [0], [n - 1], None, 0)
        check(ctx, n, [0], [n - 1], bits_of([2.5]), n - 1)   # from the far end: nothing is reached


def test_path_many_buckets(ctx):
    n = 5000
    rows, cols = np.arange(n - 1), np.arange(1, n)
    w = np.arange(1, n, dtype=np.float64)
    st, (dist, parent, _) = check(ctx, n, rows, cols, bits_of(w), 0)
    assert dist[-1] == w.sum() and st[3] == n - 1
    ctx.set_option("sssp_delta_log2", 0)   # width 1.0: every vertex is a bucket of its own, most buckets are empty
    try:
        st, _ = check(ctx, n, rows, cols, bits_of(w), 0)
        assert st[0] == n and st[1] == n   # one vertex per launch (the last one has no entry to relax), nothing re-inserted
    finally:
        ctx.set_option("sssp_delta_log2", AUTO)


def test_path_of_zero_weights_is_one_bucket(ctx):
    n = 5000
    rows, cols = np.arange(n - 1), np.arange(1, n)
    st, (dist, parent, _) = check(ctx, n, rows, cols, bits_of(np.zeros(n - 1)), 0)
    assert not dist.any() and st[3] == n - 1 and np.array_equal(parent[1:], np.arange(n - 1))


def test_zero_weight_cycles_do_not_trap_the_parents(ctx):
    # src 0 -> 1 (1.0); 1 <-> 2 at 0.0 (a 2-cycle); 0 -> 3 (2.0); 3 -> 4 -> 5 -> 3 at 0.0 (a triangle); 5 -> 6 (1.0)
    rows = [0, 1, 2, 0, 3, 4, 5, 5]
    cols = [1, 2, 1, 3, 4, 5, 3, 6]
    w = [1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0]
    st, (dist, parent, _) = check(ctx, 7, rows, cols, bits_of(w), 0)
    assert list(parent) == [0, 0, 1, 0, 3, 4, 5]
    for v in range(7):   # every chain ends at the source
        x, steps = v, 0
        while x != 0:
            x, steps = parent[x], steps + 1
            assert steps <= 7


def test_absorbed_weights_and_negative_zero(ctx):
    # 1e-20 disappears in 1.0 + 1e-20: 1 <-> 2 look like a zero-weight 2-cycle at distance 1.0, both directions present
    rows = [0, 0, 1, 2, 2, 3, 1]
    cols = [1, 2, 2, 1, 3, 2, 3]
    w = [1.0, 1.0, 1e-20, 1e-20, 1.0, 1e-20, -0.0]
    st, (dist, parent, _) = check(ctx, 4, rows, cols, bits_of(w), 0)
    assert list(dist) == [0.0, 1.0, 1.0, 1.0] and list(parent) == [0, 0, 0, 1]
    # from 3 the tiny weights are all there is: they add up
    st, (dist, parent, _) = check(ctx, 4, rows, cols, bits_of(w), 3)
    assert dist[2] == 1e-20 and dist[1] == 2e-20 and np.isinf(dist[0])


def test_infinite_and_overflowing_routes_are_skipped(ctx):
    inf = float("inf")
    st, (dist, parent, _) = check(ctx, 3, [0, 1], [1, 2], bits_of([1.0, inf]), 0)
    assert np.isinf(dist[2]) and parent[2] == -1
    # 0 -> 1 -> 4 overflows (1e308 + 1e308); 0 -> 2 -> 3 -> 4 is longer and finite
    rows = [0, 1, 0, 2, 3]
    cols = [1, 4, 2, 3, 4]
    w = [1e308, 1e308, 5e307, 5e307, 5e307]
    st, (dist, parent, _) = check(ctx, 5, rows, cols, bits_of(w), 0)
    assert dist[4] == 5e307 + 5e307 + 5e307 and parent[4] == 3


def test_hub_rows(ctx):
    d = HUB_DEG + 37
    pre, post = 10, 10
    centre = pre
    n = pre + 1 + d + post
    leaves = np.arange(centre + 1, centre + 1 + d)
    chain = np.arange(centre + 1, n - 1)
    rows = np.concatenate([np.arange(pre), np.full(d, centre), chain])
    cols = np.concatenate([np.arange(1, pre + 1), leaves, chain + 1])   # a path into the centre, the star, the leaves and a tail chained on
    w = hashed(rows, cols, "int")
    bits = bits_of(w)
    W = upload(ctx, n, rows, cols, bits)
    st, (dist, parent, _) = check(ctx, n, rows, cols, bits, centre, W)   # the hub is the source
    assert np.isinf(dist[:pre]).all() and np.isfinite(dist[centre:]).all()
    st, (dist, parent, _) = check(ctx, n, rows, cols, bits, 0, W)        # the hub is in the middle of every path
    assert np.isfinite(dist).all() and (parent[leaves] == centre).sum() > 1
    W.free()
    Wb = upload(ctx, n, rows, cols, None)
    check(ctx, n, rows, cols, None, 0, Wb)
    Wb.free()


@pytest.fixture(scope="module")
def random_graph():
    rng = np.random.default_rng(0x555B)
    n = 3000
    rows, cols = random_pairs(rng, n, 20000, lo=1)   # vertex 0 is isolated
    return n, rows, cols, rng.integers(1, 6, len(rows)).astype(np.float64), rng.random(len(rows))


@pytest.mark.parametrize("kind", ["ties", "uniform"])
def test_random_graphs(ctx, random_graph, kind):
    n, rows, cols, wt, wu = random_graph
    bits = bits_of(wt if kind == "ties" else wu)
    W = upload(ctx, n, rows, cols, bits)
    for src in (int(rows[0]), n - 1, 0):
        st, (dist, parent, _) = check(ctx, n, rows, cols, bits, src, W)
        if src == 0:
            assert np.isinf(dist[1:]).all() and st[1] == 1
        else:
            assert np.isfinite(dist).sum() > n // 2
    W.free()


def hypersparse(ctx, m, vals):
    """The same entries stored as a delta layer stores them: the ids of the non-empty rows + a row-pointer array over those."""
    rp, ci, _ = m.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(m.nrows, m.ncols, short, ci, vals, hyper_rows=rows)


@pytest.mark.parametrize("kind", ["int", "unit"])
def test_rmat14_dense_and_hypersparse(ctx, kind):
    A = ctx.mat_rmat(14)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.repeat(np.arange(n), deg)
    cols = ci.astype(np.int64)
    bits = bits_of(hashed(rows, cols, kind))
    W = ctx.mat_from_csr(n, n, rp, ci, bits)
    H = hypersparse(ctx, A, bits)
    for src in (int(np.argmax(deg)), int(np.nonzero(deg == 1)[0][0])):
        want = sssp(n, rows, cols, bits, src)
        got = engine.sssp(ctx, W, src, stats=True)
        same(got, want)
        goth = engine.sssp(ctx, H, src, stats=True)
        same(goth, want)
        assert np.array_equal(got[0].view(U64), goth[0].view(U64)) and np.array_equal(got[1], goth[1])
    for m in (W, H, A):
        m.free()


def test_bool_matrix_is_bfs(ctx, random_graph):
    n, rows, cols, _, _ = random_graph
    A = upload(ctx, n, rows, cols, None)
    At = A.transpose()
    src = int(rows[0])
    level, _, _ = engine.bfs(ctx, A, At, src)
    dist, parent, st = engine.sssp(ctx, A, src, stats=True)
    want = np.where(level < 0, np.inf, level.astype(np.float64))
    assert np.array_equal(dist.view(U64), want.view(U64))
    assert st[3] == level.max()
    # parent[v] = the smallest in-neighbour one level up
    up = (level[rows] >= 0) & (level[rows] + 1 == level[cols])
    best = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(best, cols[up], rows[up])
    best[best == np.iinfo(np.int64).max] = -1
    best[src] = src
    assert np.array_equal(parent, best)
    _, _, depth = sssp(n, rows, cols, None, src)
    assert np.array_equal(depth, level.astype(np.int64))
    A.free()
    At.free()


def test_deterministic_under_every_bucket_width(ctx, random_graph):
    n, rows, cols, wt, wu = random_graph
    src = int(rows[0])
    for w in (wt, wu):
        bits = bits_of(w)
        W = upload(ctx, n, rows, cols, bits)
        want = sssp(n, rows, cols, bits, src)
        runs = [engine.sssp(ctx, W, src, stats=True), engine.sssp(ctx, W, src, stats=True)]
        assert ctx.get_option("sssp_delta_log2") == AUTO
        auto = ctx.get_option("sssp_last_delta_log2")
        assert -8 <= auto <= 8
        try:
            for k in (-30, AUTO, 1023):   # a tiny width, the default, a width wider than every distance
                ctx.set_option("sssp_delta_log2", k)
                assert ctx.get_option("sssp_delta_log2") == k
                runs.append(engine.sssp(ctx, W, src, stats=True))
                assert ctx.get_option("sssp_last_delta_log2") == (auto if k == AUTO else k)
        finally:
            ctx.set_option("sssp_delta_log2", AUTO)
        for got in runs:
            same(got, want)
        W.free()
    for bad in (-1075, 1024, 4097):
        with pytest.raises(FgpuError):
            ctx.set_option("sssp_delta_log2", bad)
    assert ctx.get_option("sssp_delta_log2") == AUTO


def test_errors_leave_the_context_usable(ctx, random_graph):
    n, rows, cols, wt, _ = random_graph
    for poison in (float("nan"), -1.0, -float("inf")):
        w = wt.copy()
        w[len(w) // 2] = poison
        W = upload(ctx, n, rows, cols, bits_of(w))
        with pytest.raises(FgpuError):
            engine.sssp(ctx, W, int(rows[0]))
        W.free()
    R = ctx.mat_from_coo(4, 5, np.array([0], dtype=U64), np.array([4], dtype=U64))
    with pytest.raises(FgpuError):
        engine.sssp(ctx, R, 0)
    R.free()
    W = upload(ctx, n, rows, cols, bits_of(wt))
    for src in (n, n + 7, 2**40):
        with pytest.raises(FgpuError):
            engine.sssp(ctx, W, src)
    check(ctx, n, rows, cols, bits_of(wt), int(rows[0]), W)
    W.free()
