"""GPU: fgpu_sssp_hops (the hop-bounded table that prunes algo.SPpaths' enumeration) against the D_h recurrence of
tests/sppaths_enum_check.py.  D_h[v] is unique, so every comparison is array equality of BIT PATTERNS, and the four counters are
compared exactly too."""
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of  # noqa: E402
from sppaths_enum_check import hop_table  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
HUB_DEG = 4096   # common.hpp
HOPS_MAX = 32    # FGPU_SSSP_HOPS_MAX
INF = float("inf")


def upload(ctx, n, rows, cols, bits):
    rows, cols = np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64)
    return ctx.mat_from_coo(n, n, rows, cols, None if bits is None else np.asarray(bits, dtype=U64))


def check(ctx, n, rows, cols, bits, src, hops, W=None):
    """run fgpu_sssp_hops, compare the table's bits and the counters with the checker; returns (table, stats)"""
    own = W is None
    if own:
        W = upload(ctx, n, rows, cols, bits)
    want, wst = hop_table(n, rows, cols, bits, src, hops)
    got, st = engine.sssp_hops(ctx, W, src, hops, stats=True)
    assert got.shape == (hops + 1, n)
    assert np.array_equal(got.view(U64), want.view(U64)), "the table differs from the checker's bits"
    assert st == wst, "the counters differ"
    plain = engine.sssp_hops(ctx, W, src, hops)
    assert np.array_equal(plain.view(U64), want.view(U64))
    if own:
        W.free()
    return got, st


def random_pairs(rng, n, m):
    a, b = rng.integers(0, n, 2 * m + 8), rng.integers(0, n, 2 * m + 8)
    key = rng.permutation(np.unique((a.astype(np.int64) * n + b)[a != b]))[:m]
    assert len(key) == m
    return key // n, key % n


def hashed(rows, cols, kind):
    """test_gpu_sssp.py's weights: a fixed hash of (row, col) as integers 1 .. 100, or as uniform doubles in [0, 1)"""
    z = (np.asarray(rows, dtype=U64) << U64(32)) ^ np.asarray(cols, dtype=U64)
    z = (z + U64(0x9E3779B97F4A7C15)) * U64(0xBF58476D1CE4E5B9)
    z ^= z >> U64(29)
    z *= U64(0x94D049BB133111EB)
    z ^= z >> U64(32)
    if kind == "int":
        return (z % U64(100) + U64(1)).astype(np.float64)
    return (z >> U64(11)).astype(np.float64) / float(1 << 53)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("hops", [0, 1, HOPS_MAX])
def test_sizes(ctx, n, hops):
    none = np.zeros(0, dtype=np.int64)
    t, st = check(ctx, n, none, none, bits_of([]), 0, hops)
    assert t[0, 0] == 0.0 and np.isinf(t[:, 1:]).all() and st[3] == min(1, hops + 1)
    check(ctx, n, none, none, None, n - 1, hops)
    if n > 1:
        t, st = check(ctx, n, [0], [n - 1], bits_of([2.5]), 0, hops)
        assert np.isinf(t[0, n - 1]) and (hops == 0 or t[hops, n - 1] == 2.5)
        check(ctx, n, [0], [n - 1], None, 0, hops)
        check(ctx, n, [0], [n - 1], bits_of([2.5]), n - 1, hops)   # from the far end: nothing is reached


def test_a_round_travels_one_arc(ctx):
    # 0 -> 1 -> 2 -> 3 at 1.0 each, and 0 -> 3 at 10.0
    t, st = check(ctx, 4, [0, 1, 2, 0], [1, 2, 3, 3], bits_of([1.0, 1.0, 1.0, 10.0]), 0, 5)
    assert t[1, 3] == 10.0 and t[2, 3] == 10.0 and t[3, 3] == 3.0 and st[3] == 4


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_chain_in_either_list_order(ctx, order):
    # 0 -> 1 -> ... -> 40 by position; the ids ascend or descend, so no processing order can hide an in-place update
    n = 41
    ids = np.arange(n) if order == "ascending" else np.arange(n)[::-1]
    rows, cols = ids[:-1], ids[1:]
    t, st = check(ctx, n, rows, cols, bits_of(np.full(n - 1, 1.0)), int(ids[0]), HOPS_MAX)
    for h in range(HOPS_MAX + 1):
        assert np.isinf(t[h, ids[h + 1:]]).all() and np.array_equal(t[h, ids[:h + 1]], np.arange(h + 1, dtype=np.float64))
    assert st[0] == HOPS_MAX and st[1] == HOPS_MAX and st[3] == HOPS_MAX + 1


def test_a_vertex_improves_in_three_rounds_and_after_a_rest(ctx):
    # vertex 9: 0 -> 9 at 100 (round 1); 0 -> 1 -> 9 at 1 + 50 (round 2); 0 -> 1 -> 2 -> 9 at 1 + 1 + 10 (round 3)
    # vertex 8: 0 -> 8 at 100 (round 1), rests in rounds 2 and 3, then 0 -> 1 -> 2 -> 3 -> 8 at 1 + 1 + 1 + 1 (round 4)
    rows = [0, 0, 1, 1, 2, 2, 0, 3]
    cols = [9, 1, 9, 2, 9, 3, 8, 8]
    w = [100.0, 1.0, 50.0, 1.0, 10.0, 1.0, 100.0, 1.0]
    t, st = check(ctx, 10, rows, cols, bits_of(w), 0, 6)
    assert list(t[:5, 9]) == [INF, 100.0, 51.0, 12.0, 12.0]
    assert list(t[:6, 8]) == [INF, 100.0, 100.0, 100.0, 4.0, 4.0] and st[3] == 5


def test_frontier_holds_a_vertex_once(ctx):
    # 0 -> 1 .. 5000 -> 5001 -> 5002: the 5000 frontier vertices of round 2 all lower 5001, which is popped once in round 3
    k = 5000
    mid = np.arange(1, k + 1)
    rows = np.concatenate([np.zeros(k, dtype=np.int64), mid, [k + 1]])
    cols = np.concatenate([mid, np.full(k, k + 1), [k + 2]])
    w = hashed(rows, cols, "int")
    t, st = check(ctx, k + 3, rows, cols, bits_of(w), 0, 4)
    assert st[1] == 1 + k + 1 + 1 and st[0] == 4 and st[3] == 4
    assert t[2, k + 1] == (w[:k] + w[k:2 * k]).min()


def test_hub_rows(ctx):
    # 0 -> a, b, c; a has exactly HUB_DEG entries, b HUB_DEG - 1, c 2 * HUB_DEG + 3: a and b are in the frontier of round 2 together
    da, db, dc = HUB_DEG, HUB_DEG - 1, 2 * HUB_DEG + 3
    a, b, c = 1, 2, 3
    leaves = 4 + np.arange(dc)
    n = 4 + dc + 1
    rows = np.concatenate([[0, 0, 0], np.full(da, a), np.full(db, b), np.full(dc, c), leaves[:100]])
    cols = np.concatenate([[a, b, c], leaves[:da], leaves[:db], leaves, np.full(100, n - 1)])
    for kind in ("int", "uniform"):
        bits = bits_of(hashed(rows, cols, kind))
        W = upload(ctx, n, rows, cols, bits)
        t, st = check(ctx, n, rows, cols, bits, 0, 4, W)
        assert np.isfinite(t[2, leaves]).all() and np.isfinite(t[3, n - 1]) and st[2] == 3 + da + db + dc + 100
        check(ctx, n, rows, cols, bits, c, 2, W)   # the hub is the source
        W.free()
    Wb = upload(ctx, n, rows, cols, None)
    check(ctx, n, rows, cols, None, 0, 3, Wb)
    Wb.free()


def test_special_weights(ctx):
    # zero weights and a zero-weight cycle 1 -> 2 -> 3 -> 1; -0.0; a self-loop on 1
    rows = [0, 1, 2, 3, 3, 1]
    cols = [1, 2, 3, 1, 4, 1]
    t, st = check(ctx, 5, rows, cols, bits_of([0.0, 0.0, -0.0, 0.0, -0.0, 5.0]), 0, 6)
    assert not t[4].any() and np.array_equal(t[4].view(U64), np.zeros(5, dtype=U64)) and st[3] == 5
    # a +inf entry is never used; 1e308 + 1e308 is skipped, the longer finite route is taken
    t, _ = check(ctx, 3, [0, 1], [1, 2], bits_of([1.0, INF]), 0, 3)
    assert np.isinf(t[:, 2]).all()
    rows = [0, 1, 0, 2, 3]
    cols = [1, 4, 2, 3, 4]
    t, _ = check(ctx, 5, rows, cols, bits_of([1e308, 1e308, 5e307, 5e307, 5e307]), 0, 4)
    assert np.isinf(t[2, 4]) and t[3, 4] == 5e307 + 5e307 + 5e307
    # a self-loop alone changes nothing
    t, st = check(ctx, 2, [0, 0], [0, 1], bits_of([0.0, 2.0]), 0, 3)
    assert t[3, 0] == 0.0 and t[3, 1] == 2.0 and st[3] == 2


def test_errors_leave_the_context_usable(ctx):
    rng = np.random.default_rng(0x40B5)
    n = 300
    rows, cols = random_pairs(rng, n, 4 * n)
    w = hashed(rows, cols, "int")
    for poison in (float("nan"), -1.0, -INF):
        bad = w.copy()
        bad[len(bad) // 2] = poison
        W = upload(ctx, n, rows, cols, bits_of(bad))
        with pytest.raises(FgpuError):
            engine.sssp_hops(ctx, W, 0, 3)
        W.free()
        with pytest.raises(ValueError):
            hop_table(n, rows, cols, bits_of(bad), 0, 3)
    R = ctx.mat_from_coo(4, 5, np.array([0], dtype=U64), np.array([4], dtype=U64))
    with pytest.raises(FgpuError):
        engine.sssp_hops(ctx, R, 0, 1)
    R.free()
    W = upload(ctx, n, rows, cols, bits_of(w))
    for src in (n, n + 7, 2**40):
        with pytest.raises(FgpuError):
            engine.sssp_hops(ctx, W, src, 3)
    for hops in (-1, HOPS_MAX + 1, 2**31 - 1):
        with pytest.raises(FgpuError):
            engine.sssp_hops(ctx, W, 0, hops)
    import ctypes as C
    assert ctx.lib.fgpu_sssp_hops(ctx._h, W._h, C.c_uint64(0), C.c_int32(1), None, None) != 0   # NULL table
    assert ctx.lib.fgpu_sssp_hops(ctx._h, None, C.c_uint64(0), C.c_int32(1), None, None) != 0
    check(ctx, n, rows, cols, bits_of(w), 0, 3, W)
    W.free()


def test_bool_matrix_gives_bfs_levels_cut_at_h(ctx):
    rng = np.random.default_rng(0xB001)
    n = 1000
    rows, cols = random_pairs(rng, n, 3 * n)
    A = upload(ctx, n, rows, cols, None)
    At = A.transpose()
    src = int(rows[0])
    level, _, _ = engine.bfs(ctx, A, At, src)
    t, _ = check(ctx, n, rows, cols, None, src, 5, A)
    for h in range(6):
        want = np.where((level < 0) | (level > h), np.inf, level.astype(np.float64))
        assert np.array_equal(t[h].view(U64), want.view(U64))
    A.free()
    At.free()


def hypersparse(ctx, m, vals):
    """the same entries as a delta layer stores them: the ids of the non-empty rows + a row-pointer array over those"""
    rp, ci, _ = m.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(m.nrows, m.ncols, short, ci, vals, hyper_rows=rows)


def test_hypersparse(ctx):
    rng = np.random.default_rng(0x4959)
    n = 5000
    rows, cols = random_pairs(rng, n, 600)   # most rows are empty
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    bits = bits_of(hashed(rows, cols, "uniform"))
    W = upload(ctx, n, rows, cols, bits)
    H = hypersparse(ctx, W, bits)
    src = int(rows[0])
    want, wst = hop_table(n, rows, cols, bits, src, 6)
    got, st = engine.sssp_hops(ctx, H, src, 6, stats=True)
    assert np.array_equal(got.view(U64), want.view(U64)) and st == wst
    W.free()
    H.free()


@pytest.fixture(scope="module", params=[300, 1000, 5000])
def random_graph(request):
    n = request.param
    rng = np.random.default_rng(0x4095 + n)
    rows, cols = random_pairs(rng, n, 4 * n)
    return n, rows, cols


@pytest.mark.parametrize("kind", ["int", "uniform"])
def test_random_graphs(ctx, random_graph, kind):
    n, rows, cols = random_graph
    bits = bits_of(hashed(rows, cols, kind))
    W = upload(ctx, n, rows, cols, bits)
    src = int(rows[0])
    for hops in (1, 2, 5, HOPS_MAX):
        check(ctx, n, rows, cols, bits, src, hops, W)
    # against fgpu_sssp: once every tight path fits into max_hops arcs, the last row is its dist, bit for bit
    dist, _, st = engine.sssp(ctx, W, src, stats=True)
    assert st[3] <= HOPS_MAX, "the graph is deeper than the test assumes"
    t = engine.sssp_hops(ctx, W, src, int(st[3]))
    assert np.array_equal(t[-1].view(U64), dist.view(U64))
    if st[3] > 1:
        assert not np.array_equal(engine.sssp_hops(ctx, W, src, 1)[-1].view(U64), dist.view(U64))
    W.free()


def test_early_stop_repeats_the_last_live_row(ctx):
    # 0 -> 1 -> 2, nothing else: round 3 lowers nothing, rows 3 .. 32 repeat row 2
    t, st = check(ctx, 70, [0, 1], [1, 2], bits_of([1.5, 2.5]), 0, HOPS_MAX)
    assert st[3] == 3 and st[0] == 3 and st[1] == 3
    assert (t[2:].view(U64) == t[2].view(U64)).all() and t[2, 2] == 4.0


def test_repeated_and_concurrent_calls_agree(ctx):
    rng = np.random.default_rng(0x7EAD)
    n = 5000
    rows, cols = random_pairs(rng, n, 4 * n)
    bits = bits_of(hashed(rows, cols, "uniform"))
    W = upload(ctx, n, rows, cols, bits)
    src = int(rows[0])
    want, _ = hop_table(n, rows, cols, bits, src, 8)
    one, two = engine.sssp_hops(ctx, W, src, 8), engine.sssp_hops(ctx, W, src, 8)
    assert np.array_equal(one.view(U64), want.view(U64)) and np.array_equal(two.view(U64), want.view(U64))
    out, errs = [None, None], []

    def work(k):
        try:
            out[k] = [engine.sssp_hops(ctx, W, src, 8) for _ in range(3)]
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for runs in out:
        for t in runs:
            assert np.array_equal(t.view(U64), want.view(U64))
    W.free()
