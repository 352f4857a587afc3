"""GPU: fgpu_maxflow (algo.maxFlow's LAGr_MaxFlow core) against tests/maxflow_check.py.  Every result goes through certify() —
a flow within the capacities, one direction per arc pair, conservation, the value at both ends, and no augmenting path left,
which by max-flow / min-cut proves optimality whatever assignment came back — and its value equals the CPU Dinic's.  All
capacities are integers or multiples of 0.25, so every comparison is exact equality; the one case that is not says so."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maxflow_check import certify, dinic, live_arcs  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
HUB_DEG = 4096   # common.hpp: rows at least this long are pushed by hub chunk


def bits_of(caps):
    return np.ascontiguousarray(caps, dtype=np.float64).view(U64)


def upload(ctx, n, rows, cols, caps):
    rows, cols = np.asarray(rows).astype(U64), np.asarray(cols).astype(U64)
    return ctx.mat_from_coo(n, n, rows, cols, None if caps is None else bits_of(caps))


def solve(ctx, n, rows, cols, caps, src, sink, M=None, exact=True, tol=0.0):
    """run fgpu_maxflow, certify the flow, compare the value with Dinic's; returns (value, rows, cols, flows, stats).
    caps None = a BOOL snapshot (capacity 1.0)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    ref = np.ones(len(rows)) if caps is None else np.asarray(caps, dtype=np.float64)
    if M is None:
        M = upload(ctx, n, rows, cols, caps)
    got = engine.maxflow(ctx, M, src, sink, stats=True)
    value, fr, fc, fv, st = got
    want = dinic(n, rows, cols, ref, src, sink)
    print(f"n={n} arcs={len(rows)} value={value!r} dinic={want!r} flow entries={len(fr)} stats={st}")
    certify(n, rows, cols, ref, src, sink, value, fr, fc, fv, exact=exact, tol=tol)
    if exact:
        assert value == want
    else:
        assert abs(value - want) <= tol
    pairs = {(min(u, v), max(u, v)) for (u, v) in live_arcs(rows, cols, ref)}
    assert st[2] == 2 * len(pairs)
    assert st[1] >= 1 if pairs else st == [0, 0, 0, 0]
    return got


def test_one_arc(ctx):
    value, fr, fc, fv, st = solve(ctx, 2, [0], [1], [2.5], 0, 1)
    assert value == 2.5 and fr.tolist() == [0] and fc.tolist() == [1] and fv.tolist() == [2.5]
    assert st[0] == 0 and st[1] == 1 and st[3] == 0   # the start saturates src's arc into the sink: no vertex is ever active
    value, fr, _, _, _ = solve(ctx, 2, [0], [1], [2.5], 1, 0)   # against the arc
    assert value == 0.0 and len(fr) == 0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_path_with_a_bottleneck_returns_the_excess_to_src(ctx, n):
    caps = np.full(n - 1, 10.0)
    caps[n // 2] = 3.25
    value, fr, fc, fv, st = solve(ctx, n, np.arange(n - 1), np.arange(1, n), caps, 0, n - 1)
    assert value == 3.25 and len(fr) == n - 1 and np.all(fv == 3.25)
    assert st[0] > 0 and st[3] > 0


# the read-out of the sorted flow (csr_edge_list): k = 1, 256 and 257 entries are one thread, exactly one workgroup of the emit
# kernel, and one element into the second
@pytest.mark.parametrize("n", [2, 257, 258])
def test_path_flow_comes_out_as_its_triples_in_order(ctx, n):
    caps = 10.0 + np.arange(n - 1) % 7
    caps[(n - 1) // 2] = 3.25   # the one strict minimum
    value, fr, fc, fv, st = solve(ctx, n, np.arange(n - 1), np.arange(1, n), caps, 0, n - 1)
    assert value == 3.25
    assert len(fr) == len(fc) == len(fv) == n - 1
    assert np.array_equal(fr, np.arange(n - 1, dtype=U64)) and np.array_equal(fc, np.arange(1, n, dtype=U64))
    assert np.all(fv == 3.25)


def test_no_path_is_zero_and_empty(ctx):
    # two islands; src's island fills up and hands everything back
    value, fr, fc, fv, st = solve(ctx, 8, [0, 1, 2, 5, 6], [1, 2, 3, 6, 7], [4.0, 3.0, 2.0, 5.0, 5.0], 0, 7)
    assert value == 0.0 and len(fr) == len(fc) == len(fv) == 0
    empty = np.zeros(0, dtype=np.int64)
    value, fr, _, _, st = solve(ctx, 5, empty, empty, np.zeros(0), 1, 3)
    assert value == 0.0 and len(fr) == 0 and st == [0, 0, 0, 0]


def test_diagonal_zero_negative_zero_and_negative_entries_are_ignored(ctx):
    rows = [0, 0, 1, 1, 1, 2, 2, 3, 0]
    cols = [0, 1, 1, 2, 3, 3, 2, 1, 3]
    caps = [9.0, 5.0, 7.0, 0.0, -0.0, 4.0, 8.0, -3.0, 1.5]
    value, fr, fc, fv, st = solve(ctx, 4, rows, cols, caps, 0, 3)
    assert value == 1.5 and fr.tolist() == [0] and fc.tolist() == [3]   # 1 -> 2 and 1 -> 3 are dead: only the direct arc carries
    assert st[2] == 6   # pairs {0,1}, {2,3}, {0,3}


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_infinite_capacities_are_invalid(ctx, bad):
    M = upload(ctx, 4, [0, 1, 3], [1, 2, 0], [1.0, 2.0, bad])   # (the bad entry is not even on a src -> sink path)
    with pytest.raises(FgpuError) as e:
        engine.maxflow(ctx, M, 0, 2)
    assert e.value.code == _ffi.FGPU_INVALID


def test_antiparallel_pairs_on_a_cycle_through_src(ctx):
    # 0 <-> 1 <-> 2 <-> 0 with both capacities positive everywhere, 1 -> 3 and 2 -> 3 into the sink
    rows = [0, 1, 1, 2, 2, 0, 1, 2, 3, 3]
    cols = [1, 0, 2, 1, 0, 2, 3, 3, 1, 2]
    caps = [5.0, 7.0, 2.5, 9.0, 6.0, 1.25, 3.0, 4.5, 2.0, 2.0]
    value, fr, fc, fv, _ = solve(ctx, 4, rows, cols, caps, 0, 3)
    assert value == 6.25   # everything that leaves src


def test_dead_end_branch_returns_its_excess(ctx):
    # main path 0 -> 1 -> 2 -> 3; off vertex 1 a chain of 40 vertices with large capacities that ends nowhere
    rows = [0, 1, 2] + [1] + list(range(4, 43))
    cols = [1, 2, 3] + [4] + list(range(5, 44))
    caps = [50.0, 2.0, 2.0] + [100.0] * 40
    value, fr, fc, fv, st = solve(ctx, 44, rows, cols, caps, 0, 3)
    assert value == 2.0 and len(fr) == 3 and st[0] > 0


@pytest.mark.parametrize("mirror", [False, True], ids=["hub-fans-out", "hub-gathers"])
def test_hub_row(ctx, mirror):
    # src -> hub -> k middle vertices -> sink (or its mirror): the hub's row has more than HUB_DEG arcs and goes by hub chunk
    k = HUB_DEG + 905
    rng = np.random.default_rng(21)
    n = k + 3
    src, hub, sink = 0, 1, 2
    mid = np.arange(3, n)
    a = rng.integers(1, 9, k).astype(np.float64)        # hub <-> middle
    b = rng.integers(0, 9, k).astype(np.float64) / 4    # middle <-> far end, some 0: dead ends the excess returns from
    total = float(np.minimum(a, b).sum())
    for big in (total + 100.0, np.floor(total / 3)):    # the hub's own arc is not / is the bottleneck
        if not mirror:   # src -big-> hub -a-> middle -b-> sink
            rows = np.concatenate([[src], np.full(k, hub), mid])
            cols = np.concatenate([[hub], mid, np.full(k, sink)])
        else:            # src -b-> middle -a-> hub -big-> sink
            rows = np.concatenate([[hub], mid, np.full(k, src)])
            cols = np.concatenate([[sink], np.full(k, hub), mid])
        caps = np.concatenate([[big], a, b])
        value, _, _, _, st = solve(ctx, n, rows, cols, caps, src, sink)
        assert value == min(big, total) and st[0] > 0


def test_bool_snapshot_equals_the_same_graph_valued_one(ctx):
    # 4 layers of 30 vertices between src and sink, random arcs from layer to layer
    rng = np.random.default_rng(22)
    L, W = 4, 30
    n = L * W + 2
    rows, cols = [np.zeros(W, dtype=np.int64)], [np.arange(W) + 2]
    for l in range(L - 1):
        key = np.unique(rng.integers(0, W * W, 70))
        rows.append(2 + l * W + key // W)
        cols.append(2 + (l + 1) * W + key % W)
    rows.append(2 + (L - 1) * W + np.arange(W))
    cols.append(np.ones(W, dtype=np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vb = solve(ctx, n, rows, cols, None, 0, 1)[0]
    vv = solve(ctx, n, rows, cols, np.ones(len(rows)), 0, 1)[0]
    assert vb == vv and vb > 0


def test_hypersparse_snapshot(ctx):
    rng = np.random.default_rng(23)
    n, m = 1 << 20, 400
    verts = rng.choice(n, 60, replace=False)
    key = np.unique(rng.integers(0, 60 * 60, m))
    rows, cols = verts[key // 60], verts[key % 60]
    caps = rng.integers(-1, 12, len(key)).astype(np.float64) / 4
    D = upload(ctx, n, rows, cols, caps)
    rp, ci, vv = D.export_csr()
    deg = np.diff(rp.astype(np.int64))
    hr = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    H = ctx.mat_from_csr(n, n, short, ci, vals=vv, hyper_rows=hr)
    src, sink = int(verts[0]), int(verts[1])
    value = solve(ctx, n, rows, cols, caps, src, sink, M=H)[0]
    assert value == solve(ctx, n, rows, cols, caps, src, sink, M=D)[0]


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_random_directed_graph(ctx, seed):
    rng = np.random.default_rng(seed)
    n, m = 2000, 10000
    key = np.unique(rng.integers(0, n * n, m + m // 50))[:m]
    key = rng.permutation(key)
    rows, cols = key // n, key % n
    caps = rng.integers(1, 101, len(key)).astype(np.float64)
    deg = np.bincount(rows, minlength=n)
    src = int(np.argmax(deg))
    deg[src] = -1
    sink = int(np.argmax(np.bincount(cols, minlength=n) * (np.arange(n) != src)))
    value, _, _, _, st = solve(ctx, n, rows, cols, caps, src, sink)
    assert value > 0 and st[0] > 0 and st[3] > 0


def test_grid_with_random_capacities(ctx):
    rng = np.random.default_rng(34)
    k = 40
    idx = np.arange(k * k).reshape(k, k)
    right = (idx[:, :-1].ravel(), idx[:, 1:].ravel())
    down = (idx[:-1, :].ravel(), idx[1:, :].ravel())
    a = np.concatenate([right[0], down[0]])
    b = np.concatenate([right[1], down[1]])
    rows, cols = np.concatenate([a, b]), np.concatenate([b, a])   # both directions, capacities of their own
    caps = rng.integers(1, 41, len(rows)).astype(np.float64) / 4
    value, _, _, _, st = solve(ctx, k * k, rows, cols, caps, 0, k * k - 1)
    assert value > 0 and st[1] >= 1


def test_super_node_capacities(ctx):
    # what the procedure builds for several sources / sinks: arcs of 2^31 - 1 out of src and into sink; sums stay below 2^53
    rng = np.random.default_rng(35)
    n, inner = 302, 300
    big = float(2**31 - 1)
    key = np.unique(rng.integers(0, inner * inner, 1500))
    rows, cols = 2 + key // inner, 2 + key % inner
    caps = rng.integers(1, 1000, len(key)).astype(np.float64)
    starts, ends = np.arange(2, 12), np.arange(200, 215)
    rows = np.concatenate([np.zeros(len(starts), dtype=np.int64), rows, ends])
    cols = np.concatenate([starts, cols, np.ones(len(ends), dtype=np.int64)])
    caps = np.concatenate([np.full(len(starts), big), caps, np.full(len(ends), big)])
    value = solve(ctx, n, rows, cols, caps, 0, 1)[0]
    assert 0 < value < big


def test_non_dyadic_capacities_within_five_decimal_places(ctx):
    """Multiples of 0.001 are not exactly representable, so sums round: the value within 5e-6 x the largest capacity of the CPU
    value — the five decimal places the reference's own flow tests allow, scaled by the largest capacity — and conservation to
    the same bound."""
    rng = np.random.default_rng(36)
    n = 500
    key = np.unique(rng.integers(0, n * n, 4000))
    rows, cols = key // n, key % n
    caps = rng.integers(1, 100000, len(key)).astype(np.float64) * 0.001
    tol = 5e-6 * float(caps.max())
    solve(ctx, n, rows, cols, caps, 3, 7, exact=False, tol=tol)


def test_error_codes(ctx):
    lib = ctx.lib
    M = upload(ctx, 4, [0, 1], [1, 2], [1.0, 1.0])
    r, c, f = _ffi.u64p(), _ffi.u64p(), C.POINTER(C.c_double)()
    k = C.c_uint64(7)
    val = C.c_double(-1.0)
    s, t = C.c_uint64(0), C.c_uint64(2)
    args = [C.byref(val), C.byref(r), C.byref(c), C.byref(f), C.byref(k)]
    assert lib.fgpu_maxflow(None, M._h, s, t, *args, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_maxflow(ctx._h, None, s, t, *args, None) == _ffi.FGPU_NULL_POINTER
    for i in range(5):
        bad = list(args)
        bad[i] = None
        assert lib.fgpu_maxflow(ctx._h, M._h, s, t, *bad, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_maxflow(ctx._h, M._h, s, t, *args, None) == _ffi.FGPU_OK and val.value == 1.0 and k.value == 2   # stats is nullable
    for p in (r, c, f):
        lib.fgpu_free(ctx._h, C.cast(p, C.c_void_p))
    with pytest.raises(FgpuError) as e:
        engine.maxflow(ctx, ctx.mat_new(3, 4), 0, 1)
    assert e.value.code == _ffi.FGPU_DIM_MISMATCH
    for src, sink in ((4, 1), (1, 4), (2**40, 0), (2, 2)):
        with pytest.raises(FgpuError) as e:
            engine.maxflow(ctx, M, src, sink)
        assert e.value.code == _ffi.FGPU_INVALID
    # nrows >= 2^32 - 1 is FGPU_INVALID in fgpu_maxflow (check_adjacency), but no constructor hands out such a snapshot: they
    # refuse the dimensions with the same code
    with pytest.raises(FgpuError) as e:
        ctx.mat_new(2**32 - 1, 2**32 - 1)
    assert e.value.code == _ffi.FGPU_INVALID
