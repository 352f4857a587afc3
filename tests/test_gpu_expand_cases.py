"""fgpu_expand_edges and fgpu_expand_trails on the inputs of tests/expand_cases.py: runs that cross a 64-entry word and a 256-lane
block in the two-layer merge (A), 64 types with stretches of empty segments and tombstoned entries (B), an irregular tree whose
childless frames sit at the scan-tile edges and batches of 4095 .. 4097 roots with 0-hop rows among them (C), used ids inside
multi-edge lists (D), the budget after every depth (E), the sort decision, the staged sort's level classes and the stability of
the second sort (F), bitmaps whose deciding bit is in the last word (G).  The expected rows come from expand_cases.trail_rows /
edge_rows, the plain reference tests/test_expand_cases_cpu.py holds against oracle.model; every column is compared for equality,
in order, and every counter the reference pins is asserted.  No engine option is set here."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_cases as ec  # noqa: E402
from test_gpu_expand_edges import Dev, bitmap, dev, single_type  # noqa: E402,F401
from test_gpu_expand_ownership import held_and_steady  # noqa: E402
from test_options_cpu import OPTIONS  # noqa: E402

pytestmark = pytest.mark.gpu
FLAGS = {"out": {}, "in": {"reversed": True}, "both": {"bidirectional": True}}
TRAIL_COLUMNS = ("row", "from", "to", "hops", "path_off", "path_node", "path_edge")
EDGE_COLUMNS = ("row", "from", "to", "id", "pass")

_KEEP, _MEMO, _BITMAP = [], {}, {}


def memo_of(g, *key):
    """one reference memo per (graph, walk parameters): the batches of a test repeat their (start, dest) rows"""
    _KEEP.append(g)                                        # (the graph is kept: its id stays its own)
    return _MEMO.setdefault((id(g),) + key, {})


def words_of(g, labels):
    _KEEP.append(g)
    key = (id(g), tuple(labels))
    if key not in _BITMAP:
        _BITMAP[key] = bitmap(g, labels)
    return _BITMAP[key]


def same(names, got, want, what):
    for name, a, w in zip(names, got, want):
        a = np.asarray(a).astype(np.int64)
        w = np.asarray(w).astype(np.int64)
        assert a.shape == w.shape, (what, name, a.shape, w.shape)
        bad = np.nonzero(a != w)[0]
        assert len(bad) == 0, (what, name, "first differing positions", bad[:5], a[bad[:5]], w[bad[:5]])


def layers_of(ctx, g, types, mt_layers):
    d = [dev(ctx, g.tensors[t], mt_layers) for t in ec.scan_of(g, types)]
    return ([x.m for x in d], [x.dp for x in d], [x.dm for x in d], [x.mt_m for x in d], [x.mt_dp for x in d], [x.mt_dm for x in d],
            [x.multi for x in d])


def any_dp(g, types):
    return any(g.tensors[t].dp for t in ec.scan_of(g, types))


def trails(ctx, g, starts, dests=None, types=(), mt_layers=False, labels=(), lo=1, hi=None, direction="out", paths=True,
           max_items=1 << 22, bm=None):
    """one fgpu_expand_trails call held against the reference: every column, every counter"""
    if bm is None and labels:
        bm = words_of(g, labels)
    res = ctx.expand_trails(starts, dests, *layers_of(ctx, g, types, mt_layers), paths=paths, min_hops=lo, max_hops=hi,
                            dst_label_bitmap=bm, max_items=max_items, **FLAGS[direction])
    want, c = ec.trail_columns(g, starts, dests, memo=memo_of(g, "t", tuple(types), hi, direction), types=types,
                               lo=lo, hi=hi, direction=direction, bitmap_nodes=ec.labelled(g, labels))
    what = (direction, lo, hi, mt_layers, paths, tuple(labels))
    assert len(res) == (8 if paths else 5)
    same(TRAIL_COLUMNS, res[:-1], want, what)
    st, rows = res[-1], len(want[0])
    assert (st[0], st[2], st[3], st[4], st[6]) == (c["frames"], c["used"], rows, c["levels"], c["multi"]), (what, st, c)
    held = (c["frames"] or len(starts)) + rows             # (no level runs under hi = 0: the roots are still held)
    assert st[5] == (1 if any_dp(g, types) else 0) and st[7] == held, (what, st, c)
    return st, rows


def edges(ctx, g, froms, tos, types=(), mt_layers=False, transposed=False, bidirectional=False, first_only=False, from_labels=(),
          to_labels=(), fbm=None, tbm=None):
    """one fgpu_expand_edges call held against the reference: the five columns, every counter.  Returns (stats, columns)"""
    assert not any(f is None and t is None for f, t in zip(froms, tos))
    fbm = words_of(g, from_labels) if fbm is None and from_labels else fbm
    tbm = words_of(g, to_labels) if tbm is None and to_labels else tbm
    res = ctx.expand_edges(froms, tos, *layers_of(ctx, g, types, mt_layers), transposed=transposed, bidirectional=bidirectional,
                           first_only=first_only, from_bitmap=fbm, to_bitmap=tbm, want_pass=True)
    want = ec.edge_columns(g, froms, tos, types=types, transposed=transposed, bidirectional=bidirectional, first_only=first_only,
                           from_nodes=ec.labelled(g, from_labels), to_nodes=ec.labelled(g, to_labels),
                           memo=memo_of(g, "e", tuple(types), transposed, bidirectional, first_only, tuple(from_labels), tuple(to_labels)))
    what = (transposed, bidirectional, first_only, mt_layers, tuple(from_labels), tuple(to_labels))
    same(EDGE_COLUMNS, res[:5], want[:, :5].T, what)
    st, c = res[-1], ec.edge_counters(want)
    T, L, P = len(ec.scan_of(g, types)), 2 if any_dp(g, types) else 1, 2 if bidirectional else 1
    assert st[7] == len(froms) * P * T * L, (what, st)
    assert st[2] == len(want)
    if len(want):
        path = 0 if T == 1 and L == 1 else (1 if len(froms) * P * g.n <= ec.ONE_KEY_LIMIT else 2)
        assert (st[4], st[5], st[6]) == (c["longest"], path, c["items"]), (what, st, c)
        if not first_only:
            assert st[3] == c["multi"], (what, st, c)
    return st, [np.array(x) for x in res[:5]]


# ---- A: the two-layer adjacency slot -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merge():
    return ec.layer_merge()


@pytest.mark.parametrize("mt_layers", [False, True], ids=["mt_structure", "mt_layers"])
@pytest.mark.parametrize("direction", ec.DIRECTIONS)
def test_a_layer_merge_trails(ctx, merge, direction, mt_layers):
    g, hubs = merge
    roots = [h[0] for h in hubs] * (direction != "in") + [h[1] for h in hubs] * (direction != "out")
    for opener in ec.A_OPENERS:                           # 0 .. 3 entries in front: every group shifts against the words
        st, rows = trails(ctx, g, [opener] + roots, None, ("T",), mt_layers, lo=1, hi=2, direction=direction)
        assert st[5] == 1 and st[6] > 0 and rows > 20000


@pytest.mark.parametrize("mt_layers", [False, True], ids=["mt_structure", "mt_layers"])
def test_a_layer_merge_edges(ctx, merge, mt_layers):
    g, hubs = merge
    froms, tos = ec.merge_edge_rows(hubs)
    for opener in ec.A_OPENERS:
        for kw in ({}, {"transposed": True}, {"bidirectional": True}, {"first_only": True},
                   {"transposed": True, "bidirectional": True, "first_only": True}):
            st, _ = edges(ctx, g, [opener] + froms, [None] + tos, ("T",), mt_layers, **kw)
            assert st[5] == 1 and st[2] > 1000


# ---- B: many types, empty stretches ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def typed():
    return ec.many_types()


ORDERS = {"ascending": ec.B_TYPES, "reversed": ec.B_TYPES[::-1]}


@pytest.mark.parametrize("order", list(ORDERS))
def test_b_many_types_trails(ctx, typed, order):
    starts = ec.many_types_rows()
    for mt_layers in (False, True):
        for direction in ec.DIRECTIONS:
            st, rows = trails(ctx, typed, starts, None, ORDERS[order], mt_layers, lo=1, hi=2, direction=direction)
            assert rows > 0 and st[6] > 0
    trails(ctx, typed, starts, [40 if i % 100 == 0 else None for i in range(len(starts))], ORDERS[order], lo=0, hi=2, direction="both",
           paths=False)


@pytest.mark.parametrize("order", list(ORDERS))
def test_b_many_types_edges(ctx, typed, order):
    rows = ec.many_types_rows()
    none = [None] * len(rows)
    for mt_layers in (False, True):
        for kw in ({}, {"first_only": True}, {"bidirectional": True}, {"bidirectional": True, "first_only": True},
                   {"transposed": True}):
            st, _ = edges(ctx, typed, rows, none, ORDERS[order], mt_layers, **kw)
            assert st[2] > 0
        edges(ctx, typed, none, rows, ORDERS[order], mt_layers)
        edges(ctx, typed, rows, [40 if i % 100 == 0 else None for i in range(len(rows))], ORDERS[order], mt_layers, first_only=True)


def test_b_sixty_five_types_are_refused(ctx, typed):
    lay = layers_of(ctx, typed, ec.B_TYPES, False)
    more = [x + x[:1] for x in lay]
    assert len(more[0]) == ec.EE_MAX_TYPES + 1
    for call in (lambda: ctx.expand_edges([0], [None], *more), lambda: ctx.expand_trails([0], None, *more, min_hops=1, max_hops=2)):
        with pytest.raises(FgpuError) as e:
            call()
        assert e.value.code == _ffi.FGPU_INVALID
    assert len(ctx.expand_edges([0], [None], *lay)[0]) > 0                      # 64 are accepted
    trails(ctx, typed, [0, 1], None, ec.B_TYPES, lo=1, hi=2)


def test_b_tombstone_run(ctx):
    g = ec.tombstones()
    live = 100 + ec.TOMB_RUN
    for mt_layers in (False, True):
        st, rows = trails(ctx, g, [0, 3], None, ("T",), mt_layers, lo=1, hi=2)
        assert rows == 2 * 3 and st[1] >= ec.TOMB_RUN + 1
        trails(ctx, g, [1, 2], None, ("T",), mt_layers, lo=1, hi=2, direction="in")
        trails(ctx, g, [0, 1, live], None, ("T",), mt_layers, lo=1, hi=3, direction="both")
        st, _ = edges(ctx, g, [0, None, live], [None, 1, None], ("T",), mt_layers)
        assert st[2] == 1 + 1 + 2 and st[0] >= ec.TOMB_RUN + 1 and st[1] >= (ec.TOMB_RUN + 1 if mt_layers else 1)
        edges(ctx, g, [0, 1, None], [None, None, 0], ("T",), mt_layers, bidirectional=True)


# ---- C: an irregular tree across scan tiles ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree():
    return ec.irregular_tree()


@pytest.mark.parametrize("lo,hi", [(1, 3), (2, 3), (3, 3), (1, 2), (0, 3)])
def test_c_irregular_tree(ctx, tree, lo, hi):
    g, sizes, _ = tree
    first2, first3 = 1 + sizes[1], 1 + sizes[1] + sizes[2]
    leaf2, leaf3 = first2 + ec.SCAN_TILE, g.n - 1             # a childless grandchild at position 4096; the last node
    for paths in (True, False):
        st, rows = trails(ctx, g, [0], None, ("T",), lo=lo, hi=hi, paths=paths)
        assert st[0] == sum(sizes[:hi]) and rows <= 120000 and st[5] == 0
        trails(ctx, g, [0], None, ("T",), labels=("K",), lo=lo, hi=hi, paths=paths)
        trails(ctx, g, [0, 0], [leaf2, leaf3], ("T",), lo=lo, hi=hi, paths=paths)
        trails(ctx, g, [leaf3, leaf2, first3], [None, 0, None], ("T",), lo=lo, hi=hi, direction="in", paths=paths)


_MANY = {}


@pytest.mark.parametrize("k", ec.MANY_ROOTS)
def test_c_many_roots_with_zero_hop_rows(ctx, k):
    g = _MANY.setdefault("g", ec.many_roots_graph())
    starts, dests = ec.many_roots(k)
    st, rows = trails(ctx, g, starts, dests, ("T",), labels=("K",), lo=0, hi=2)
    assert rows > k // 3
    trails(ctx, g, starts, dests, ("T",), labels=("K",), lo=0, hi=2, direction="both", paths=False)
    trails(ctx, g, starts, dests, ("T",), labels=("K",), lo=0, hi=0)


# ---- D: used edges inside id lists -----------------------------------------------------------------------------------------
def test_d_used_ids_inside_lists(ctx):
    pair = ec.parallel_pair(4)
    st, rows = trails(ctx, pair, [0, 1], None, ("T",), lo=1, hi=None, direction="both")
    assert rows == 2 * ec.trails_between_two(4) == 2 * 64
    ring = ec.parallel_ring(3, 3)
    for direction in ec.DIRECTIONS:
        trails(ctx, pair, [0, 1], None, ("T",), lo=0, hi=3, direction=direction)
        st, rows = trails(ctx, ring, [0, 1, 2], None, ("T",), lo=1, hi=4, direction=direction)
        assert direction == "both" or rows == 3 * ec.RING_TRAILS                # (both ways: the reference alone)
        trails(ctx, ring, [0, 1, 2], [0, None, 1], ("T",), lo=0, hi=4, direction=direction, paths=False)
    lists = ec.id_lists()
    st, rows = trails(ctx, lists, [0], None, ("T",), lo=1, hi=2, direction="both")
    assert rows == sum(ec.LISTS) + sum(L * (L - 1) for L in ec.LISTS) and st[2] == sum(ec.LISTS)
    trails(ctx, lists, [0], None, ("T",), lo=1, hi=2)
    trails(ctx, lists, [1, 2, 3, 4, 0], None, ("T",), lo=1, hi=2, direction="in")
    trails(ctx, lists, [1, 2, 3, 4], None, ("T",), lo=1, hi=2, direction="both")


# ---- E: the budget per level -----------------------------------------------------------------------------------------------
def test_e_budget_after_every_depth(ctx):
    g = ec.budget_tree()
    starts, k, hi = [0, 0], 2, ec.E_DEPTH
    layers = layers_of(ctx, g, ("T",), False)

    def refused(max_items):
        got = []
        with pytest.raises(FgpuError) as e:
            ctx.expand_trails(starts, None, *layers, paths=True, min_hops=1, max_hops=hi, max_items=max_items, stats_out=got)
        assert e.value.code == _ffi.FGPU_INSUFFICIENT_SPACE
        return got

    for d in range(hi):
        held = ec.held_after(d, k=k)
        if d + 1 < hi:                                     # depth d fits exactly; the next depth does not
            st = refused(held)
            assert st[7] == ec.held_after(d + 1, k=k) > held and st[4] == d + 2, (d, st)
        else:
            st, rows = trails(ctx, g, starts, None, ("T",), lo=1, hi=hi, max_items=held)
            assert st[7] == held and st[4] == hi
        st = refused(held - 1)
        assert st[7] == held > held - 1 and st[4] == d + 1, (d, st)
        trails(ctx, g, starts, None, ("T",), lo=1, hi=hi)                       # the next ordinary call is correct


# ---- F: the sort decision and the key-space classes ------------------------------------------------------------------------
_SORT = {}


def sort_graph(n):
    return _SORT.setdefault(n, ec.sort_graph(n))


@pytest.mark.parametrize("name,n,k,bidir,path,levels", ec.key_space_cases()[:6], ids=[c[0] for c in ec.key_space_cases()[:6]])
def test_f_key_space_classes(ctx, name, n, k, bidir, path, levels):
    g = sort_graph(n)
    rows = ec.key_space_rows(n, k)
    st, _ = edges(ctx, g, rows, [None] * k, ec.F_TYPES, bidirectional=bidir)
    assert st[5] == path == 1 and st[2] > k
    edges(ctx, g, rows, [None] * k, ec.F_TYPES, mt_layers=True, bidirectional=bidir, first_only=True)


def test_f_sort_switch_keeps_the_common_rows(ctx):
    (_, n, k1, _, p1, _), (_, n2, k2, _, p2, _) = ec.key_space_cases()[6:]
    assert n == n2 and k2 == k1 + 1 and (p1, p2) == (1, 2) and k1 * n == ec.ONE_KEY_LIMIT
    g = sort_graph(n)
    rows = ec.key_space_rows(n, k2)
    st1, one = edges(ctx, g, rows[:k1], [None] * k1, ec.F_TYPES)
    st2, two = edges(ctx, g, rows, [None] * k2, ec.F_TYPES)
    assert (st1[5], st2[5]) == (1, 2)
    common = two[0] < k1
    for a, b in zip(one, two):
        assert np.array_equal(a, b[common])


@pytest.mark.parametrize("n_ent", ec.STABLE_ENT)
def test_f_second_sort_is_stable(ctx, n_ent):
    g = ec.stable_graph(n_ent)
    st, _ = edges(ctx, g, list(ec.STABLE_ROWS), [None] * len(ec.STABLE_ROWS), ec.F_TYPES)
    assert st[5] == 2 and st[0] == n_ent and st[1] == 0 and st[3] > 0
    st, _ = edges(ctx, g, list(ec.STABLE_ROWS), [None] * len(ec.STABLE_ROWS), ec.F_TYPES, first_only=True)
    assert st[5] == 2 and st[2] == n_ent // 3 + n_ent % 3


# ---- G: bitmaps at word edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.G_SIZES)
def test_g_bitmap_word_edges(ctx, n):
    g, special = ec.word_edge_graph(n)
    none = [None] * len(special)
    for dirty in (False, True):
        F, Q = bitmap(g, ["F"]), bitmap(g, ["Q"])
        if dirty:
            F, Q = ec.dirty_bits(F, n), ec.dirty_bits(Q, n)
            assert n % 64 == 0 or int(F[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1
        for kw in ({}, {"bidirectional": True}, {"transposed": True}):
            st, _ = edges(ctx, g, special, none, ("T",), from_labels=("F",), fbm=F, **kw)
            assert st[2] > 0
            edges(ctx, g, special, none, ("T",), to_labels=("Q",), tbm=Q, **kw)
            edges(ctx, g, none, special, ("T",), from_labels=("F",), to_labels=("Q",), fbm=F, tbm=Q, **kw)
        for direction in ec.DIRECTIONS:
            st, rows = trails(ctx, g, special, None, ("T",), labels=("F",), lo=0, hi=2, direction=direction, bm=F)
            assert rows > 0
            trails(ctx, g, special, [n - 1] * len(special), ("T",), labels=("Q",), lo=0, hi=1, direction=direction, bm=Q, paths=False)


# ---- the file leaves nothing behind ----------------------------------------------------------------------------------------
def test_z_options_at_default_and_device_memory_steady(ctx, merge, typed):
    defaults = {name: default for name, _, _, _, default in OPTIONS}
    for name, default in defaults.items():
        assert ctx.get_option(name) == default, name
    g, hubs = merge
    froms, tos = ec.merge_edge_rows(hubs)
    tree = ec.budget_tree()
    sg = sort_graph(64)
    wg, special = ec.word_edge_graph(65)
    lists = ec.id_lists()
    mr = _MANY.setdefault("g", ec.many_roots_graph())
    starts, dests = ec.many_roots(300)
    one_per_family = [
        lambda: trails(ctx, g, [h[1] for h in hubs], None, ("T",), True, lo=1, hi=2, direction="in")[0],
        lambda: edges(ctx, g, froms, tos, ("T",), True, bidirectional=True)[0],
        lambda: trails(ctx, typed, ec.many_types_rows(), None, ec.B_TYPES, lo=1, hi=2, direction="both")[0],
        lambda: trails(ctx, mr, starts, dests, ("T",), labels=("K",), lo=0, hi=2)[0],
        lambda: trails(ctx, lists, [0], None, ("T",), lo=1, hi=2, direction="both")[0],
        lambda: trails(ctx, tree, [0, 0], None, ("T",), lo=1, hi=ec.E_DEPTH, max_items=ec.held_after(ec.E_DEPTH - 1, k=2))[0],
        lambda: edges(ctx, sg, ec.key_space_rows(64, 9), [None] * 9, ec.F_TYPES)[0],
        lambda: trails(ctx, wg, special, None, ("T",), labels=("F",), lo=0, hi=2, direction="both")[0],
    ]
    for call in one_per_family:
        call()                                             # (the device tensors of the case are built)
        held_and_steady(ctx, call)
