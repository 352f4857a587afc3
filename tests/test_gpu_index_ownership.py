"""GPU: every index a snapshot caches goes when the snapshot goes, and attaching one changes no result.

Each case warms its path once on matrices of its own (lane pools, staging), reads `device_bytes()`, creates the matrices
again, makes the index attach, frees the matrices (and any plan), and `in_use` must be back at the value read; the result of
the call that attached the index must equal the warm-up's, which ran on a fresh copy.  Where the index is the only thing a
call can have left behind, `in_use` must also have grown while the matrices were still alive: the index did attach.

The graph has 8192 vertices: out-degree 16 everywhere, one row (HUB_ROW) with 4096 more out-edges and one column (HUB_COL)
with 4096 more in-edges.  That is the smallest size at which the hub list and the finer push list are both non-empty for A and
for A' (HUB_DEG = 4096, PUSH_HUB_DEG = 1024), the partitioned count hop has eight full partitions of 1024 rows, and bp_to_csr
and the item split (BP_ITEM = 256) both run."""
import numpy as np
import pytest

from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64 = np.uint64

N = 8192
D = 16
HUB_ROW, HUB_COL = 5, 7
NLAYER = 300


def _edges():
    v = np.repeat(np.arange(N, dtype=np.int64), D)
    j = np.tile(np.arange(D, dtype=np.int64), N)
    rows = np.concatenate([v, np.full(4096, HUB_ROW), np.arange(4096, N)])
    cols = np.concatenate([(v + 1 + 509 * j) % N, np.arange(4096), np.full(4096, HUB_COL)])
    return rows.astype(U64), cols.astype(U64)


ROWS, COLS = _edges()
_RNG = np.random.default_rng(0x1DE5)
_PICK = _RNG.choice(len(ROWS), NLAYER, replace=False)
DM_ROWS, DM_COLS = ROWS[_PICK], COLS[_PICK]                      # tombstones of existing edges
DP_ROWS, DP_COLS = _RNG.integers(0, N, NLAYER, dtype=U64), _RNG.integers(0, N, NLAYER, dtype=U64)
# 130 source rows (more than two words of bits per vertex), the hub row among them: the state the count hop reads is dense
SRC = np.concatenate([[HUB_ROW], _RNG.choice(np.arange(64, N), 129, replace=False)]).astype(U64)
FRONTIER = _RNG.integers(0, 2**64, N // 64, dtype=U64)           # about half of the vertices


def test_the_graph_is_what_the_cases_need():
    deg = np.bincount(ROWS.astype(np.int64), minlength=N)
    indeg = np.bincount(COLS.astype(np.int64), minlength=N)
    assert len(np.unique(ROWS * U64(N) + COLS)) >= len(ROWS) - D - D        # the hub edges repeat at most D edges each
    assert deg.min() >= D and deg[HUB_ROW] >= 4096 and indeg[HUB_COL] >= 4096
    assert np.sort(deg)[-2] < 1024 and np.sort(indeg)[-2] < 1024            # one hub each way, nothing else on any list
    assert N % 128 == 0 and N // 8 == 1024


def _plain(x):
    """a call's result as something `==` compares: arrays as bytes, containers element-wise"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(_plain(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _plain(v)) for k, v in sorted(x.items()))
    return x


def adjacency(ctx):
    return ctx.mat_from_coo(N, N, ROWS, COLS)


def layers(ctx):
    return ctx.mat_from_coo(N, N, DP_ROWS, DP_COLS), ctx.mat_from_coo(N, N, DM_ROWS, DM_COLS)


def in_use(ctx):
    ctx.sync()
    return ctx.device_bytes()[0]


def comes_and_goes(ctx, case):
    """`case()` creates its matrices, attaches, frees, and returns its result: warmed once, then run between two readings"""
    first = _plain(case())
    before = in_use(ctx)
    second = _plain(case())
    assert in_use(ctx) == before
    assert second == first
    return second


def test_hub_lists_and_pull_order_through_a_plan(ctx):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        made = in_use(ctx)
        plan = engine.BfsPlan(ctx, A, At)
        plan.run(HUB_ROW)
        level, _ = plan.fetch()
        stats = plan.stats()
        reached = (stats["levels"], stats["reached"])
        plan.free()
        assert in_use(ctx) > made          # pull_col stays on A'
        At.free()
        A.free()
        assert level[HUB_ROW] == 0 and level.max() >= 2 and (level >= 0).all() and reached[1] == N
        return level, reached
    comes_and_goes(ctx, case)


@pytest.mark.parametrize("first_freed", ["A", "At"])
def test_the_cached_one_call_plan(ctx, first_freed):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        made = in_use(ctx)
        level, _, _ = engine.bfs(ctx, A, At, HUB_ROW, want_parent=False)
        again, _, _ = engine.bfs(ctx, A, At, HUB_COL, want_parent=False)        # the cached plan serves it
        assert in_use(ctx) > made          # the plan and pull_col
        for m in ((A, At) if first_freed == "A" else (At, A)):
            m.free()
        return level, again
    comes_and_goes(ctx, case)


def _pull(ctx, A, At):
    return engine.vxm(ctx, FRONTIER, None, A, At, direction=3)


def test_the_tiled_layout(ctx):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        want = engine.vxm(ctx, FRONTIER, None, A, At, direction=2)
        made = in_use(ctx)
        info = At.build_tiles(10, 2, 1)
        assert (info["tile_bits"], info["tiles"], info["groups"], info["vec"], info["k"]) == (10, 8, 128, 2, 1)
        got = _pull(ctx, A, At)
        assert in_use(ctx) > made
        assert np.array_equal(got, want)
        At.free()
        A.free()
        return info, got
    comes_and_goes(ctx, case)


def test_the_blocked_layout(ctx):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        want = engine.vxm(ctx, FRONTIER, None, A, At, direction=2)
        made = in_use(ctx)
        with ctx.options(tiled_layout=2):
            got = _pull(ctx, A, At)        # the first dense pull builds it
        info = At.tiles_info()
        assert info["tile_bits"] == 18 and info["tiles"] == 1
        assert in_use(ctx) > made
        assert np.array_equal(got, want)
        At.free()
        A.free()
        return info, got
    comes_and_goes(ctx, case)


def test_a_layout_rebuilt_over_the_other(ctx):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        want = engine.vxm(ctx, FRONTIER, None, A, At, direction=2)
        out = []
        tiled = At.build_tiles(10, 2, 1)
        out.append(_pull(ctx, A, At))
        held = in_use(ctx)
        with ctx.options(tiled_layout=2):
            blocked = At.build_tiles()     # blocked over tiled
        out.append(_pull(ctx, A, At))
        assert blocked["tile_bits"] == 18
        assert At.build_tiles(10, 2, 1) == tiled      # tiled over blocked
        out.append(_pull(ctx, A, At))
        assert in_use(ctx) == held         # the same layout as before holds the same blocks: the blocked one went whole
        assert all(np.array_equal(w, want) for w in out)
        At.free()
        A.free()
        return tiled, blocked, out
    comes_and_goes(ctx, case)


def test_wordrow_through_a_merge(ctx):
    def case():
        A = adjacency(ctx)
        DP, DM = layers(ctx)
        made = in_use(ctx)
        M = A.merge(DP, DM)
        out = M.export_csr()[:2]
        a, dp, dm = (r * U64(N) + c for r, c in ((ROWS, COLS), (DP_ROWS, DP_COLS), (DM_ROWS, DM_COLS)))
        assert M.nvals == len(np.union1d(np.setdiff1d(a, dm), dp)) < A.nvals + NLAYER
        M.free()
        assert in_use(ctx) > made          # wordrow stays on the three layers
        for m in (DM, DP, A):
            m.free()
        return out
    comes_and_goes(ctx, case)


def test_the_cached_transpose_and_its_items_through_a_count(ctx):
    def case():
        A = adjacency(ctx)
        DP, DM = layers(ctx)
        made = in_use(ctx)
        with ctx.options(expand_mode=2):
            clean = engine.expand_count(ctx, SRC, [A, A])
            dirty = engine.expand_count(ctx, SRC, [A, A], dp=[DP, DP], dm=[DM, DM])
            rp, dest, _ = engine.expand(ctx, SRC, [A, A])          # bp_to_csr
        assert in_use(ctx) > made
        with ctx.options(expand_mode=1):
            assert engine.expand_count(ctx, SRC, [A, A])[:2] == clean[:2]
        assert clean[0] == len(dest) == rp[-1]
        for m in (DM, DP, A):
            m.free()
        return clean, dirty, rp, dest
    comes_and_goes(ctx, case)


def test_the_four_partitioned_plans_on_one_matrix(ctx):
    def case():
        A = adjacency(ctx)
        with ctx.options(expand_mode=1):
            want = engine.expand_count(ctx, SRC, [A, A])
        out = []
        with ctx.options(expand_mode=2, expand_xcd_min_mb=0):
            for direct in (0, 1):
                for dense in (0, 1):
                    with ctx.options(expand_xp_direct=direct, expand_xp_dense=dense):
                        held = in_use(ctx)
                        folds = ctx.get_option("expand_xp_slot_folds") + ctx.get_option("expand_xp_piece_folds")
                        out.append(engine.expand_count(ctx, SRC, [A, A]))
                        assert ctx.get_option("expand_xp_slot_folds") + ctx.get_option("expand_xp_piece_folds") > folds   # partitioned
                        assert in_use(ctx) > held       # this pair's plan joined the others
        assert all(o[:2] == want[:2] for o in out)
        A.free()
        return out
    comes_and_goes(ctx, case)


def test_the_cached_transpose_alone_through_betweenness(ctx):
    def case():
        A = adjacency(ctx)                 # never expanded: no item list on its transpose
        made = in_use(ctx)
        with ctx.options(bc_direction=2):
            cent, stats = engine.betweenness(ctx, A, SRC[:8], stats=True)
        assert in_use(ctx) > made
        At = A.transpose()
        with ctx.options(bc_direction=2):
            given, _ = engine.betweenness(ctx, A, SRC[:8], At=At)
        assert np.array_equal(cent, given)
        At.free()
        A.free()
        return cent, stats
    comes_and_goes(ctx, case)


def test_the_column_ranges_through_pagerank(ctx):
    def case():
        A = adjacency(ctx)
        At = A.transpose()
        with ctx.options(pagerank_parts=0):
            want = engine.pagerank(ctx, A, At)
        made = in_use(ctx)
        with ctx.options(pagerank_parts=2):
            got = engine.pagerank(ctx, A, At)
        assert in_use(ctx) > made
        assert got[1] == want[1]
        np.testing.assert_allclose(got[0], want[0], rtol=1e-6, atol=0)    # (the bound of tests/test_gpu_pagerank.py)
        At.free()
        A.free()
        return got
    comes_and_goes(ctx, case)


def test_a_stream_of_wide_destinations_closed_unread(ctx):
    def case():
        A = adjacency(ctx)
        read = engine.ExpandStream(ctx, SRC, [A, A], chunk_rows=16, dest_bits=64)       # 130 rows: 9 chunks over the 4 slots
        got = [(first, rp.copy(), d.copy()) for first, rp, d in read]
        read.close()
        made = in_use(ctx)                 # (whatever the chain attaches to A is there now)
        s = engine.ExpandStream(ctx, SRC, [A, A], chunk_rows=16, dest_bits=64)
        assert in_use(ctx) > made          # the result and the slots' staging
        out = (s.nnz, s.flops)
        s.close()
        assert in_use(ctx) == made
        assert sum(len(d) for _, _, d in got) == out[0]
        A.free()
        return out, got
    comes_and_goes(ctx, case)
