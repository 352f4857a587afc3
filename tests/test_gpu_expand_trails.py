"""fgpu_expand_trails (csrc/expand_trails.hip): CondVarLenTraverse for a whole batch.  The expected rows always come from
oracle.model.var_len_expand, called per distinct (start, dest) over the same tensors and concatenated with the row index in
front; every column — row, from, to, hops and, under PATHS, the offsets, nodes and edges of every path — is compared for
equality, in order.  Shapes are the smallest at which a kernel can go wrong: a level past 65 536 items (past 16-bit indices, one
workgroup and one wordrow word), a 70 000-entry hub inside the walk, 70 000 rows, hypersparse layers at n = 2^20, trails of 64
and 65 edges."""
import numpy as np
import pytest

from falkordb_amd import _ffi, host
from falkordb_amd._ffi import FgpuError

from oracle import model
from test_gpu_expand_edges import bitmap, dev, random_graph, single_type
from test_gpu_expand_ownership import held_and_steady
from test_gpu_host import _twin_graphs
from trails_check import graph_of, random_multigraph

pytestmark = pytest.mark.gpu
U64 = np.uint64
MULTI = model.MULTI_EDGE
DIRECTIONS = ({}, {"reversed": True}, {"bidirectional": True})


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def scan_of(g, types):
    return [g.type_ids[t] for t in types if t in g.type_ids] if types else list(range(len(g.tensors)))


def call(ctx, g, starts, dests, types=(), mt_layers=False, dst_labels=(), emit_path=True, with_mt=True, **kw):
    d = [dev(ctx, g.tensors[t], mt_layers) for t in scan_of(g, types)]
    mt = lambda xs: xs if with_mt else None
    return ctx.expand_trails(starts, dests, [x.m for x in d], [x.dp for x in d], [x.dm for x in d], mt([x.mt_m for x in d]),
                             mt([x.mt_dp for x in d]), mt([x.mt_dm for x in d]), [x.multi for x in d], paths=emit_path,
                             dst_label_bitmap=bitmap(g, dst_labels) if dst_labels else None, **kw)


def want_columns(g, starts, dests, types=(), dst_labels=(), min_hops=1, max_hops=None, reversed=False, bidirectional=False):
    """(row, from, to, hops, path_off, path_node, path_edge) of the oracle, one oracle call per DISTINCT (start, dest)"""
    memo = {}
    cols = [[] for _ in range(6)]
    for i, s in enumerate(starts):
        key = (int(s), None if dests is None else dests[i])
        if key not in memo:
            rows = model.var_len_expand(g, key[0], list(types), dest=key[1], min_hops=min_hops, max_hops=max_hops, reversed=reversed,
                                        bidirectional=bidirectional, dst_labels=dst_labels, emit_path=True)
            memo[key] = (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64),
                         np.array([(len(r[2]) - 1) // 2 for r in rows], dtype=np.int64),
                         np.array([v for r in rows for v in r[2][0::2]], dtype=np.int64),
                         np.array([e for r in rows for e in r[2][1::2]], dtype=np.int64))
        f, t, h, pn, pe = memo[key]
        for c, a in zip(cols, (np.full(len(f), i, dtype=np.int64), f, t, h, pn, pe)):
            c.append(a)
    row, f, t, h, pn, pe = [np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols]
    return row, f, t, h, np.concatenate([[0], np.cumsum(h)]).astype(np.int64) if len(h) else np.zeros(0, dtype=np.int64), pn, pe


def check(ctx, g, starts, dests=None, types=(), mt_layers=False, dst_labels=(), emit_path=True, max_items=1 << 22, lo=1, hi=None, **kw):
    res = call(ctx, g, starts, dests, types, mt_layers, dst_labels, emit_path, min_hops=lo, max_hops=hi, max_items=max_items, **kw)
    want = want_columns(g, starts, dests, types, dst_labels, lo, hi, **kw)
    names = ("row", "from", "to", "hops", "path_off", "path_node", "path_edge")
    for name, got, w in zip(names, res[:-1], want):
        got = got.astype(np.int64)
        assert got.shape == w.shape, (name, got.shape, w.shape)
        bad = np.nonzero(got != w)[0]
        assert len(bad) == 0, (name, bad[:5], got[bad[:5]], w[bad[:5]])
    st = res[-1]
    assert st[3] == len(want[0])
    return st, len(want[0])


# ---- random multigraphs ------------------------------------------------------------------------------------------------
HOPS = ((1, 1), (1, 3), (2, 4), (0, 2), (0, 0))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_clean_random_multigraphs(ctx, seed):
    g, _ = random_multigraph(np.random.default_rng(seed))
    starts = [0, 3, 7, 3, 8, 1]
    total = 0
    for kw in DIRECTIONS:
        for (lo, hi) in HOPS:
            for dests in (None, [2, None, 7, 3, 2, 2]):
                st, n = check(ctx, g, starts, dests, lo=lo, hi=hi, **kw)
                assert st[5] == 0, "no dp layer: the entry positions are the adjacency order"
                total += n
        check(ctx, g, starts, types=["KNOWS"], dst_labels=["L"], hi=3, **kw)
        check(ctx, g, starts, types=["LIKES", "KNOWS", "LIKES"], hi=2, emit_path=False, **kw)
    assert total > 500
    ga, _ = random_multigraph(np.random.default_rng(100 + seed), acyclic=True)
    for kw in ({}, {"reversed": True}):
        check(ctx, ga, list(range(9)), lo=1, hi=None, **kw)
        check(ctx, ga, list(range(9)), [5] * 9, lo=1, hi=None, **kw)


@pytest.fixture(scope="module")
def layered():
    """three types over shared pairs, every tensor with unfolded deltas: a dp entry shadowing an m entry with another id, dp-only
    pairs, tombstones, tombstoned and re-added pairs, pending multi-edges, self-loops"""
    return random_graph(5, 12, 16, loops=2)


@pytest.mark.parametrize("mt_layers", [False, True])
@pytest.mark.parametrize("types", [("C", "A", "B"), ("B", "A", "B"), ()], ids=["CAB", "BAB", "all"])
def test_layered_random_multigraphs(ctx, layered, types, mt_layers):
    starts = [0, 5, 11, 5, 2]
    for kw in DIRECTIONS:
        for (lo, hi) in ((1, 1), (1, 2), (2, 3), (0, 2)):
            st, _ = check(ctx, layered, starts, None, types, mt_layers, lo=lo, hi=hi, **kw)
            assert st[5] == 1 and st[6] > 0
            check(ctx, layered, starts, [3, 5, None, 0, 2], types, mt_layers, lo=lo, hi=hi, **kw)
        check(ctx, layered, starts, None, types, mt_layers, dst_labels=["P"], hi=2, **kw)


def test_dirty_single_type_every_delta_kind(ctx):
    m = {(1, 2): 10, (1, 3): 11, (1, 4): MULTI, (2, 5): 12, (1, 9): 13, (8, 1): 14, (9, 1): 15, (1, 1): 16, (4, 12): 17}
    dp = {(1, 2): 20, (1, 6): 21, (1, 7): MULTI, (7, 1): 22, (4, 12): 23, (11, 1): MULTI}
    dm = {(1, 3), (9, 1), (4, 12)}
    me = {(1, 4): [40, 41], (1, 7): [30, 31, 32], (11, 1): [50, 51]}
    g = single_type(64, m, me, dp, dm)
    for mt_layers in (False, True):
        for kw in DIRECTIONS:
            st, n = check(ctx, g, list(range(13)), None, ["T"], mt_layers, lo=1, hi=3, **kw)
            assert st[5] == 1 and n > 13


# ---- trail shapes --------------------------------------------------------------------------------------------------------
def test_trail_shapes(ctx):
    tri = graph_of(3, [("R", 0, 1), ("R", 1, 2), ("R", 2, 0)])
    for kw in DIRECTIONS:                                           # walked to exhaustion: every edge once
        st, n = check(ctx, tri, [0, 1, 2], lo=0, hi=None, **kw)
        assert n == (3 * (1 + 6) if kw.get("bidirectional") else 3 * (1 + 3))
        check(ctx, tri, [0, 1, 2], [0, 1, 0], lo=1, hi=None, **kw)    # dest == start: the cycles
    par = graph_of(2, [("R", 0, 1), ("R", 0, 1)])                   # two parallel edges: two trails, each edge once
    st, n = check(ctx, par, [0, 1], lo=1, hi=None, bidirectional=True)
    assert n == 2 * 4 and st[2] == 2 * 2 * (1 + 2)                  # per trail: one used id met after its first edge, two after both
    for kw in DIRECTIONS:
        check(ctx, par, [0, 1], lo=1, hi=3, **kw)
    loop = graph_of(2, [("R", 0, 0), ("R", 0, 1)])                  # a self-loop in each direction mode
    for kw in DIRECTIONS:
        st, n = check(ctx, loop, [0, 1, 0], lo=0, hi=None, **kw)
        check(ctx, loop, [0, 1], [0, 0], lo=1, hi=None, **kw)
    edge = graph_of(2, [("R", 0, 1)])                               # immediate back-tracking over the same edge is refused
    st, n = check(ctx, edge, [0, 1], lo=1, hi=5, bidirectional=True)
    assert n == 2 and st[2] == 2


# ---- size edges --------------------------------------------------------------------------------------------------------
def test_level_past_65536_items(ctx):
    """20 children reached over 15 parallel edges each = 300 frames at depth 1, each with 300 entries: 90 000 entries,
    candidates and emissions in one level"""
    n = 1 + 20 + 20 * 300
    pairs, me, eid = {}, {}, 10**6
    for c in range(20):
        pairs[(0, 1 + c)] = MULTI
        me[(0, 1 + c)] = list(range(eid, eid + 15))
        eid += 15
        for j in range(300):
            pairs[(1 + c, 21 + 300 * c + j)] = eid
            eid += 1
    g = single_type(n, pairs, me)
    st, rows = check(ctx, g, [0], types=["T"], lo=2, hi=2)
    assert rows == 90000 and st[0] == 301 and st[1] == 20 + 90000 and st[4] == 2
    st, rows = check(ctx, g, [0], types=["T"], lo=1, hi=2)
    assert rows == 300 + 90000
    st, rows = check(ctx, g, [0], types=["T"], lo=2, hi=2, emit_path=False)
    assert rows == 90000


def test_hub_inside_the_walk(ctx):
    n = 70002
    pairs = {(0, 1): 5, (0, 2): 6}
    pairs.update({(1, 2 + j): 100 + j for j in range(70000)})
    g = single_type(n, pairs)
    st, rows = check(ctx, g, [0], types=["T"], lo=1, hi=2)
    assert rows == 2 + 70000 and st[1] == 2 + 70000
    check(ctx, g, [70001, 5], types=["T"], lo=1, hi=2, reversed=True)


@pytest.mark.parametrize("k", [1024, 70000])
def test_many_rows_and_duplicates(ctx, k):
    g, _ = random_multigraph(np.random.default_rng(3))
    starts = [(0, 3, 3, 7, 8)[i % 5] for i in range(k)]            # 3 twice in a row: duplicate rows
    st, rows = check(ctx, g, starts, lo=1, hi=2, bidirectional=k == 1024, max_items=1 << 24)
    assert rows > k and st[0] > k
    if k == 1024:
        check(ctx, g, starts, [(2, None, 3)[i % 3] for i in range(k)], lo=0, hi=3)


def test_hypersparse_layers(ctx):
    n = 1 << 20
    base = [7, 70000, 500000, n - 1, n - 2, 3]
    pairs = {(base[i], base[(i + 1) % 6]): 10 + i for i in range(6)}
    pairs[(7, n - 1)] = MULTI
    dp = {(70000, 7): 40, (7, 70000): 41}
    g = single_type(n, pairs, {(7, n - 1): [50, 51]}, dp, {(3, 7)})
    for kw in DIRECTIONS:
        for mt_layers in (False, True):
            check(ctx, g, [7, n - 1, 12345], None, ["T"], mt_layers, lo=0, hi=4, **kw)


# ---- depth ---------------------------------------------------------------------------------------------------------------
def chain(edges):
    return single_type(edges + 1, {(i, i + 1): 100 + i for i in range(edges)})


def test_depth_limit(ctx):
    st, rows = check(ctx, chain(64), [0], types=["T"], lo=1, hi=None)
    assert rows == 64 and st[4] == 65
    check(ctx, chain(64), [64], types=["T"], lo=60, hi=None, reversed=True)
    with pytest.raises(FgpuError) as e:
        call(ctx, chain(65), [0], None, ["T"], min_hops=1, max_hops=None)
    assert e.value.code == _ffi.FGPU_INSUFFICIENT_SPACE
    st, rows = check(ctx, chain(65), [0], types=["T"], lo=1, hi=64)
    assert rows == 64
    st, rows = check(ctx, chain(65), [0], types=["T"], lo=1, hi=65)   # the frames at depth 64 still emit
    assert rows == 65


# ---- the 0-hop row and empty calls -------------------------------------------------------------------------------------
def test_zero_hops_and_empty_calls(ctx):
    g, _ = random_multigraph(np.random.default_rng(4))
    # n_types == 0: only the 0-hop rows, the dest test applied
    row, f, t, hops, off, pn, pe, st = ctx.expand_trails([3, 5, 3], [None, 5, 4], [], paths=True, min_hops=0, max_hops=3)
    assert list(row) == [0, 1] and list(f) == [3, 5] == list(t) and list(hops) == [0, 0]
    assert list(off) == [0, 0, 0] and list(pn) == [3, 5] and len(pe) == 0 and st[0] == 0 and st[3] == 2
    assert len(ctx.expand_trails([3, 5], None, [], min_hops=1, max_hops=3)[0]) == 0
    st, rows = check(ctx, g, [0, 3], lo=3, hi=2)                     # min_hops > max_hops
    assert rows == 0
    st, rows = check(ctx, g, [0, 3, 4], [None, 2, 4], lo=0, hi=0)    # max_hops == 0
    assert rows == 2 and st[0] == 0
    check(ctx, g, list(range(9)), lo=0, hi=0, dst_labels=["L"])
    st, rows = check(ctx, g, [], lo=0, hi=2)                         # k == 0
    assert rows == 0


# ---- the budget ----------------------------------------------------------------------------------------------------------
def test_budget(ctx):
    g, _ = random_multigraph(np.random.default_rng(5))
    starts = [0, 3, 7, 8]
    st, rows = check(ctx, g, starts, lo=0, hi=4, bidirectional=True)
    peak = st[7]
    assert peak == st[0] + st[3] and peak > rows                    # every frame and every emission is held
    st2, _ = check(ctx, g, starts, lo=0, hi=4, bidirectional=True, max_items=peak)     # exactly at the budget
    assert st2 == st
    got = []
    with pytest.raises(FgpuError) as e:
        call(ctx, g, starts, None, min_hops=0, max_hops=4, bidirectional=True, max_items=peak - 1, stats_out=got)
    assert e.value.code == _ffi.FGPU_INSUFFICIENT_SPACE
    assert got[7] > peak - 1 and 0 < got[0] <= st[0] and got[4] <= st[4]
    with pytest.raises(FgpuError) as e:                                                # not even the roots fit
        call(ctx, g, starts, None, min_hops=1, max_hops=4, max_items=3)
    assert e.value.code == _ffi.FGPU_INSUFFICIENT_SPACE
    check(ctx, g, starts, lo=0, hi=4, bidirectional=True)                               # the next call is correct


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_invalid_calls_leave_the_context_usable(ctx):
    g, _ = random_multigraph(np.random.default_rng(6))
    d = [dev(ctx, t) for t in g.tensors]
    m, mt = [x.m for x in d], [x.mt_m for x in d]
    multi = [x.multi for x in d]
    bool_m = ctx.mat_from_coo(9, 9, np.array([1], dtype=U64), np.array([2], dtype=U64), None)
    wide = ctx.mat_new(10, 10)
    tall = ctx.mat_new(9, 10)
    has_multi = [i for i, x in enumerate(d) if x.multi is not None]
    assert has_multi
    no_table = list(multi)
    no_table[has_multi[0]] = None
    multi_start = next(s for (s, _), ids in g.tensors[has_multi[0]].me.items() if len(ids) > 1)
    base = dict(min_hops=1, max_hops=2)
    bad = [
        lambda: ctx.expand_trails([9], None, m, mt_m=mt, multi=multi, **base),                        # start at n
        lambda: ctx.expand_trails([0], [9], m, mt_m=mt, multi=multi, **base),                         # dest at n
        lambda: ctx.expand_trails([0], None, [tall, m[1]], multi=multi, **base),                      # non-square
        lambda: ctx.expand_trails([0], None, [m[0], wide], multi=multi, **base),                      # mismatched
        lambda: ctx.expand_trails([0], None, [m[0], m[1]], dp=[wide, None], multi=multi, **base),     # mismatched dp
        lambda: ctx.expand_trails([0], None, [bool_m, m[1]], multi=multi, **base),                    # unvalued m
        lambda: ctx.expand_trails([0], None, m, multi=multi, reversed=True, **base),                  # no mt_m, incoming walked
        lambda: ctx.expand_trails([0], None, m, multi=multi, bidirectional=True, **base),
        lambda: ctx.expand_trails([0], None, m, mt_m=[mt[0], None], multi=multi, bidirectional=True, **base),
        lambda: ctx.expand_trails([0], None, m * 33, multi=multi * 33, **base),                       # 66 types
        lambda: ctx.expand_trails([0], None, m, mt_m=mt, multi=multi, reversed=True, bidirectional=True, **base),
        lambda: ctx.expand_trails([multi_start], None, m, mt_m=mt, multi=no_table, **base),            # MULTI_EDGE without a row
        lambda: ctx.expand_trails([0], None, m, multi=multi, max_items=0, **base),
        lambda: ctx.expand_trails([0], None, m, multi=multi, max_items=(1 << 32) - 1, **base),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(FgpuError) as e:
            f()
        assert e.value.code == _ffi.FGPU_INVALID, (i, e.value)
        check(ctx, g, [0, 3], lo=1, hi=2)
    # unknown flag bits and too many rows: through the raw entry
    import ctypes as C
    n = C.c_uint64()
    outs = [_ffi.u32p() for _ in range(4)]
    one = np.zeros(1, dtype=U64)
    args = lambda k, flags: (ctx._h, one.ctypes.data_as(_ffi.u64p), None, k, None, None, None, None, None, None, None, 0, flags, 0, 1,
                             None, 1 << 22, *[C.byref(o) for o in outs], None, None, None, C.byref(n), None)
    assert ctx.lib.fgpu_expand_trails(*args(1, 8)) == _ffi.FGPU_INVALID
    assert ctx.lib.fgpu_expand_trails(*args((1 << 24) + 1, 0)) == _ffi.FGPU_INVALID
    poff = _ffi.u64p()                                                                               # a path pointer without PATHS
    a = list(args(1, 0))
    a[21] = C.byref(poff)
    assert ctx.lib.fgpu_expand_trails(*a) == _ffi.FGPU_INVALID
    check(ctx, g, [0, 3], lo=1, hi=2)
    for x in (bool_m, wide, tall):
        x.free()


# ---- ownership and the counters ----------------------------------------------------------------------------------------
def test_keeps_no_device_memory(ctx, layered):
    g, _ = random_multigraph(np.random.default_rng(7))
    for gg, types in ((g, ()), (layered, ("C", "A", "B"))):
        call(ctx, gg, [0, 3, 7], None, types, min_hops=0, max_hops=3, bidirectional=True)      # (the device tensors are built)
        for kw in (dict(), dict(reversed=True), dict(bidirectional=True, emit_path=False)):
            held_and_steady(ctx, lambda: call(ctx, gg, [0, 3, 7], None, types, min_hops=0, max_hops=3, **kw))

    def refused():
        with pytest.raises(FgpuError):
            call(ctx, g, [0, 3, 7], None, min_hops=0, max_hops=4, bidirectional=True, max_items=40)
        return 0

    held_and_steady(ctx, refused)


def test_frames_equal_the_host_dfs(ctx, hctx):
    rng = np.random.default_rng(8)
    edges = [(("KNOWS", "LIKES")[int(rng.integers(0, 2))], int(rng.integers(0, 9)), int(rng.integers(0, 9))) for _ in range(16)]
    edges += [edges[0], edges[3]]
    hg, og = _twin_graphs(hctx, 9, edges)
    starts = [0, 3, 7, 3]
    for kw in DIRECTIONS:
        for (lo, hi) in ((1, 1), (1, 3), (0, 2), (2, 4)):
            for dests in (None, [2, 2, 2, 2]):
                st, _ = check(ctx, og, starts, dests, lo=lo, hi=hi, **kw)
                frames = sum(hg.var_len_traverse(s, dest=None if dests is None else dests[i], min_hops=lo, max_hops=hi, prune=False,
                                                 **kw)[1]["frames"] for i, s in enumerate(starts))
                assert st[0] == frames, (kw, lo, hi, dests)
