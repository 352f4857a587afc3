"""fgpu_node_degrees (csrc/degrees.hip): indegree() / outdegree() for a batch of nodes and for the whole graph.  The expected
value is a one-pass count over the oracle tensors' effective structure (1 per inline pair, the list length per multi-edge pair),
held on a sample of nodes to oracle.model.node_relationships, and on every batch to the rows fgpu_expand_edges emits for the
same nodes.  Shapes are the smallest at which a pass can go wrong: rows of 0, 1, 63, 64, 65, 300 and 5000 entries, lists of 2,
65 and 300 ids, 1 / 2 / 64 types, batches of 0, 1, 257 and 70 000 positions, windows, hypersparse layers and ids at 2^32 - 3."""
import gc
from collections import Counter

import numpy as np
import pytest

from falkordb_amd import _ffi

from oracle import model

pytestmark = pytest.mark.gpu
U64 = np.uint64
MULTI = model.MULTI_EDGE
OUT, IN = _ffi.FGPU_DEGREE_OUT, _ffi.FGPU_DEGREE_IN


# ---- the oracle's tensors on the device (as tests/test_gpu_expand_edges.py puts them there) ---------------------------------
def _coo(ctx, n, entries, valued):
    keys = sorted(entries)
    if not keys:
        return None
    r = np.array([k[0] for k in keys], dtype=U64)
    c = np.array([k[1] for k in keys], dtype=U64)
    return ctx.mat_from_coo(n, n, r, c, np.array([entries[k] for k in keys], dtype=U64) if valued else None)


def flat(me):
    keys = sorted(k for k in me if len(me[k]) >= 2)
    off = np.concatenate([[0], np.cumsum([len(me[k]) for k in keys])]).astype(U64)
    ids = np.array([x for k in keys for x in me[k]], dtype=U64)
    return np.array([(s << 32) | d for s, d in keys], dtype=U64), off, ids


class Dev:
    """One oracle Tensor as the call takes it.  mt_layers=False: mt_m is the transposed STRUCTURE, clean; True: mt_m = m',
    mt_dm = (dm & m)', mt_dp = dp' — layers that overlap, as a transposed tensor with pending deltas may hold them."""

    def __init__(self, ctx, T, mt_layers=False):
        n = T.nrows
        self.m = _coo(ctx, n, T.m, True) or ctx.mat_new(n, n)
        self.dp = _coo(ctx, n, T.dp, True)
        self.dm = _coo(ctx, n, {k: 1 for k in T.dm}, False)
        tr = lambda keys: {(c, r): 1 for r, c in keys}
        if mt_layers:
            self.mt_m = _coo(ctx, n, tr(T.m), False) or ctx.mat_new(n, n)
            self.mt_dp = _coo(ctx, n, tr(T.dp), False)
            self.mt_dm = _coo(ctx, n, tr(k for k in T.dm if k in T.m), False)
        else:
            self.mt_m = _coo(ctx, n, tr(T.structure()), False) or ctx.mat_new(n, n)
            self.mt_dp = self.mt_dm = None
        self.multi = ctx.multi_new(*flat(T.me)) if any(len(v) >= 2 for v in T.me.values()) else None


_DEV, _WANT = {}, {}


def dev(ctx, T, mt_layers=False):
    key = (id(T), mt_layers)
    if key not in _DEV:
        _DEV[key] = (T, Dev(ctx, T, mt_layers))   # (the tensor is kept: its id stays its own)
    return _DEV[key][1]


def want_counts(T):
    """(out, in) Counters of one tensor: one pass over its effective structure, computed once and left unchanged"""
    if id(T) not in _WANT:
        o, i = Counter(), Counter()
        for s, d in T.structure():
            c = len(T.get(s, d))
            o[s] += c
            i[d] += c
        _WANT[id(T)] = (T, o, i)
    return _WANT[id(T)][1:]


def layer_args(ctx, tensors, mt_layers=False, with_mt=True, multi=True):
    d = [dev(ctx, T, mt_layers) for T in tensors]
    mt = lambda name: [getattr(x, name) for x in d] if with_mt else None
    return ([x.m for x in d], [x.dp for x in d], [x.dm for x in d], mt("mt_m"), mt("mt_dp"), mt("mt_dm"),
            [x.multi for x in d] if multi else None)


def check(ctx, g, types, nodes, mt_layers=False, expand=True):
    """out, in and both on one batch (nodes None: the whole graph) against the one-pass count and fgpu_expand_edges' rows;
    returns the stats of the call that asked for both"""
    tensors = [g.tensors[g.type_ids[t]] for t in types]
    args = layer_args(ctx, tensors, mt_layers)
    ids = list(range(g.n)) if nodes is None else [int(v) for v in nodes]
    want_o = np.array([sum(want_counts(T)[0][v] for T in tensors) for v in ids], dtype=U64)
    want_i = np.array([sum(want_counts(T)[1][v] for T in tensors) for v in ids], dtype=U64)
    k, nt = len(ids), len(tensors)
    o, none, st = ctx.node_degrees(nodes, *args, out=True, incoming=False)
    assert none is None and np.array_equal(o, want_o), np.nonzero(o != want_o)[0][:5]
    assert st[5] == int(want_o.sum()) and st[6] == 0 and st[2] == 0
    none, i, st = ctx.node_degrees(nodes, *args, out=False, incoming=True)
    assert none is None and np.array_equal(i, want_i), np.nonzero(i != want_i)[0][:5]
    assert st[6] == int(want_i.sum()) and st[5] == 0 and st[1] == 0
    o, i, st = ctx.node_degrees(nodes, *args, out=True, incoming=True)
    assert np.array_equal(o, want_o) and np.array_equal(i, want_i)
    assert st[5] == int(want_o.sum()) and st[6] == int(want_i.sum())
    assert st[0] <= 2 * k * nt and st[0] % max(k, 1) == 0
    if st[0] == 2 * k * nt:
        assert st[1] == st[2] == 0, "nothing is walked when the row pointers answer every triple"
    if expand and k and nt:   # the contract: the rows fgpu_expand_edges emits for from = node / to = node
        row = ctx.expand_edges(ids, [None] * k, *args)[0]
        assert np.array_equal(np.bincount(row, minlength=k).astype(U64), want_o)
        row = ctx.expand_edges([None] * k, ids, *args)[0]
        assert np.array_equal(np.bincount(row, minlength=k).astype(U64), want_i)
    return st


def check_oracle(g, types, nodes):
    """the one-pass count against oracle.model.node_relationships on at most 40 distinct nodes (it sorts the structure per call)"""
    tensors = [g.tensors[g.type_ids[t]] for t in types]
    for v in list(dict.fromkeys(int(x) for x in nodes))[:40]:
        assert len(model.node_relationships(g, v, types, True, False)) == sum(want_counts(T)[0][v] for T in tensors)
        assert len(model.node_relationships(g, v, types, False, True)) == sum(want_counts(T)[1][v] for T in tensors)


# ---- graphs ------------------------------------------------------------------------------------------------------------
def single_type(n, pairs, me=None, dp=None, dm=None):
    g = model.Graph(n)
    g.add_type("T")
    g.tensors[0] = model.Tensor(n, n, m=pairs, dp=dp, dm=dm, me=me)
    g.adjacency.m = g.tensors[0].structure()
    return g


ROW_NODE = {0: 10, 1: 11, 63: 12, 64: 13, 65: 14, 300: 15, 5000: 16}   # row length -> the node that has it
COL_NODE = {65: 21, 300: 22, 5000: 20}                                   # column length -> node


def _rows_and_columns():
    pairs = {}
    for length, v in ROW_NODE.items():
        for j in range(length):
            pairs[(v, 100 + j)] = 10**6 * v + j
    for length, v in COL_NODE.items():
        for j in range(length):
            pairs[(200 + j, v)] = 10**6 * v + j
    pairs[(30, 30)] = 5                                                 # an inline self-loop
    return pairs


@pytest.fixture(scope="module")
def plain():
    """clean layers and no multi-edge: every (position, type, direction) is the row-pointer tier's"""
    return single_type(6000, _rows_and_columns())


@pytest.fixture(scope="module")
def lists():
    """the same rows and columns with id lists of 2, 65 and 300 and a multi-edge self-loop: the table sends every entry
    through the entry tier"""
    pairs = _rows_and_columns()
    me = {(12, 100): [7, 8], (13, 101): list(range(1000, 1065)), (15, 102): list(range(2000, 2300)),
          (200, 20): list(range(3000, 3065)), (31, 31): [90, 91, 92]}
    for p in me:
        pairs[p] = MULTI
    return single_type(6000, pairs, me)


SHAPE_NODES = list(ROW_NODE.values()) + list(COL_NODE.values()) + [30, 31, 100, 102, 200, 5199, 5999, 0]


@pytest.fixture(scope="module")
def dirty():
    """unfolded deltas: a dp pair shadowing an m pair, a dp-only pair, a dp value of MULTI_EDGE, dm tombstones on an inline and
    on a multi-edge pair, a tombstoned pair that dp re-adds, an inline self-loop in m and a multi-edge one in dp"""
    m = {(1, 2): 10, (1, 3): 11, (1, 4): MULTI, (2, 5): 12, (1, 9): 13, (8, 1): 14, (9, 1): 15, (1, 1): 16, (4, 12): 17,
         (2, 6): MULTI}
    dp = {(1, 2): 20, (1, 6): 21, (1, 7): MULTI, (7, 1): 22, (4, 12): 23, (11, 1): MULTI, (5, 5): MULTI}
    dm = {(1, 3), (9, 1), (4, 12), (2, 6)}
    me = {(1, 4): [40, 41], (1, 7): [30, 31, 32], (11, 1): [50, 51], (2, 6): [60, 61, 62], (5, 5): [70, 71]}
    return single_type(64, m, me, dp, dm)


def random_graph(seed, n, npairs, ntypes=3, loops=8, deltas=True):
    """ntypes tensors over shared pairs, a quarter of the pairs multi-edge, every tensor with unfolded deltas of all four kinds
    (deltas=False: committed pairs only), some self-loops"""
    rng = np.random.default_rng(seed)
    g = model.Graph(n)
    eid = [1000]

    def fresh(k=1):
        eid[0] += k
        return list(range(eid[0] - k, eid[0]))

    cand = [(int(a), int(b)) for a, b in rng.integers(0, n, (npairs, 2))] + [(int(v), int(v)) for v in rng.integers(0, n, loops)]
    cand = list(dict.fromkeys(cand))
    for t in range(ntypes):
        g.add_type("ABCDEFG"[t])
        m, dp, dm, me = {}, {}, set(), {}
        for j, p in enumerate(cand):
            if rng.random() < 0.45:
                continue
            kind = int(rng.integers(0, 10)) if deltas else 0
            ids = fresh(int(rng.integers(2, 5))) if j % 4 == 0 else fresh()
            val = ids[0] if len(ids) == 1 else MULTI
            if kind < 6:
                m[p] = val                                # committed
            elif kind == 6:
                dp[p] = val                               # pending, dp only
            elif kind == 7:
                m[p] = fresh()[0]
                dm.add(p)                                 # tombstoned: no edge
                continue
            elif kind == 8:
                m[p] = fresh()[0]
                dp[p] = val                               # shadowed: dp's value wins
            else:
                m[p] = fresh()[0]
                dm.add(p)
                dp[p] = val                               # tombstoned and re-added
            if val == MULTI:
                me[p] = ids
        g.tensors[t] = model.Tensor(n, n, m=m, dp=dp, dm=dm, me=me)
    g.adjacency.m = set().union(*[t.structure() for t in g.tensors])
    return g


@pytest.fixture(scope="module")
def rnd():
    return random_graph(11, 60, 260)


# ---- row lengths, list lengths, directions -------------------------------------------------------------------------------
def test_clean_layers_are_answered_from_the_row_pointers(ctx, plain):
    check_oracle(plain, ["T"], SHAPE_NODES)
    st = check(ctx, plain, ["T"], SHAPE_NODES)
    assert st[0] == 2 * len(SHAPE_NODES) and st[1] == st[2] == 0 and st[3] == st[4] == 0 and st[7] == 1
    o, i, st = ctx.node_degrees([ROW_NODE[k] for k in ROW_NODE], *layer_args(ctx, plain.tensors))
    assert o.tolist() == list(ROW_NODE) and i is None and st[0] == len(ROW_NODE)
    o, i, st = ctx.node_degrees([COL_NODE[k] for k in COL_NODE] + [30], *layer_args(ctx, plain.tensors), out=False, incoming=True)
    assert i.tolist() == list(COL_NODE) + [1] and o is None


def test_rows_and_lists_through_the_entry_tier(ctx, lists):
    check_oracle(lists, ["T"], SHAPE_NODES)
    st = check(ctx, lists, ["T"], SHAPE_NODES)
    assert st[0] == 0, "a table sends both directions of the type through the entry tier"
    nnz_out = sum(ROW_NODE) + 3 + 1 + 2     # the rows, 200's three entries into the column nodes, (5199, 20), the two loops
    assert st[1] == nnz_out and st[3] == 2 * 5 - 1 and st[4] == 300    # ((13, 101) is met from one side only: 101 is not asked)
    args = layer_args(ctx, lists.tensors)
    o, _, st = ctx.node_degrees([12, 13, 15, 31, 30], *args)
    assert o.tolist() == [63 + 1, 64 + 64, 300 + 299, 3, 1] and st[3] == 4 and st[4] == 300
    _, i, st = ctx.node_degrees([20, 100, 101, 102, 31, 30], *args, out=False, incoming=True)
    assert i.tolist() == [4999 + 65, 5 + 2, 4 + 65, 4 + 300, 3, 1] and st[2] == 5000 + 6 + 5 + 5 + 1 + 1 and st[4] == 300


@pytest.mark.parametrize("mt_layers", [False, True])
def test_dirty_layers(ctx, dirty, mt_layers):
    nodes = list(range(13))
    check_oracle(dirty, ["T"], nodes)
    st = check(ctx, dirty, ["T"], nodes, mt_layers)
    assert st[1] > 0 and st[2] > 0 and st[4] == 3
    args = layer_args(ctx, dirty.tensors, mt_layers)
    o, i, _ = ctx.node_degrees([1, 2, 5, 4], *args, incoming=True)
    # 1 -> 2 (dp's id), 4 (2 ids), 9, 1, 6, 7 (3 ids); (1, 3) is tombstoned.  2 -> 5 only: the multi-edge (2, 6) is tombstoned
    assert o.tolist() == [1 + 2 + 1 + 1 + 1 + 3, 1, 2, 1]
    # into 1: 8, 1 (the loop), 7, 11 (2 ids); (9, 1) is tombstoned.  Into 5: 2 and the loop's 2 ids
    assert i.tolist() == [1 + 1 + 1 + 2, 1, 1 + 2, 2]


# ---- types ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt_layers", [False, True])
def test_one_two_and_sixty_four_types(ctx, rnd, mt_layers):
    nodes = list(range(60))
    loops = [s for s, d in rnd.adjacency.m if s == d]
    assert loops
    check_oracle(rnd, ["C", "A", "B"], nodes)
    for types in (["A"], ["C", "A"], ["B", "B"], ["C", "A", "B"]):          # B twice counts twice
        check(ctx, rnd, types, nodes, mt_layers)
    many = [("A", "B", "C")[j % 3] for j in range(64)]
    st = check(ctx, rnd, many, nodes + [59, 0, 59], mt_layers)
    assert st[7] == 1


def test_no_type_and_sixty_five_types(ctx, rnd):
    o, i, st = ctx.node_degrees([3, 4, 2**40], [], incoming=True)
    assert o.tolist() == [0, 0, 0] and i.tolist() == [0, 0, 0] and st == [0] * 8
    args = layer_args(ctx, [rnd.tensors[0]] * 65)
    with pytest.raises(_ffi.FgpuError) as e:
        ctx.node_degrees([1], *args)
    assert e.value.code == _ffi.FGPU_INVALID
    check(ctx, rnd, ["A"], [1, 2])


# ---- batch sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 257, 70000])
def test_batch_sizes_with_repeated_ids(ctx, lists, k):
    cycle = (15, 13, 13, 10, 21, 31, 102, 5999)                              # (13 twice in a row)
    nodes = [cycle[j % len(cycle)] for j in range(k)]
    st = check(ctx, lists, ["T"], nodes)
    assert st[7] == (1 if k else 0)


# ---- the whole-graph form --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g3001():
    return random_graph(5, 3001, 4000, ntypes=2)


def test_whole_graph_in_three_windows(ctx, g3001):
    found = ctx.get_option("degree_window_rows")
    assert found == 1 << 24
    try:
        ctx.set_option("degree_window_rows", 1024)
        check_oracle(g3001, ["B", "A"], [0, 1023, 1024, 2047, 2048, 3000] + list(range(30)))
        st = check(ctx, g3001, ["B", "A"], None)
        assert st[7] == 3
        st = check(ctx, g3001, ["A"], list(range(3001)))                    # the batch form walks the same windows
        assert st[7] == 3
        for bad in (63, (1 << 24) + 1):
            with pytest.raises(_ffi.FgpuError) as e:
                ctx.set_option("degree_window_rows", bad)
            assert e.value.code == _ffi.FGPU_INVALID and ctx.get_option("degree_window_rows") == 1024
    finally:
        ctx.set_option("degree_window_rows", found)


def test_whole_graph_of_70001_nodes(ctx):
    g = random_graph(9, 70001, 30000, ntypes=1)
    check_oracle(g, ["A"], [0, 70000] + [s for s, _ in sorted(g.adjacency.m)[:30]])
    st = check(ctx, g, ["A"], None)
    assert st[7] == 1 and st[1] > 0
    clean = random_graph(9, 70001, 30000, ntypes=1, deltas=False)
    d = dev(ctx, clean.tensors[0])
    o, i, st = ctx.node_degrees(None, [d.m], mt_m=[d.mt_m], incoming=True)   # no table given: entries are counted, not read
    want_o, want_i = Counter(s for s, _ in clean.tensors[0].m), Counter(t for _, t in clean.tensors[0].m)
    assert o.tolist() == [want_o[v] for v in range(70001)] and i.tolist() == [want_i[v] for v in range(70001)]
    assert st[0] == 2 * 70001 and st[1] == st[2] == 0 and st[7] == 1
    # k must be the dimension
    with pytest.raises(_ffi.FgpuError) as e:
        raw(ctx, None, 70000, [d.m], OUT)
    assert e.value.code == _ffi.FGPU_INVALID


# ---- hypersparse layers, wide ids -----------------------------------------------------------------------------------------
def _sparse_graph(n, rows, seed, top=()):
    rng = np.random.default_rng(seed)
    g = model.Graph(n)
    eid = 5
    for t in range(2):
        g.add_type("AB"[t])
        m, dp, dm, me = {}, {}, set(), {}
        for r in rows:
            for c in sorted(set(rng.integers(0, n, int(rng.integers(1, 6))).tolist())) + [int(rows[0])] + list(top):
                if rng.random() < 0.2:
                    me[(r, c)] = [eid, eid + 1, eid + 2]
                    m[(r, c)] = MULTI
                else:
                    m[(r, c)] = eid
                eid += 3
        if t == 1:
            keys = sorted(m)
            for p in keys[:20]:
                dm.add(p)
            for p in keys[20:40]:
                dp[p] = eid
                eid += 1
            dp[(int(rows[1]), 12345)] = eid
        g.tensors[t] = model.Tensor(n, n, m=m, dp=dp, dm=dm, me={p: v for p, v in me.items() if p not in dp})
    g.adjacency.m = g.tensors[0].structure() | g.tensors[1].structure()
    return g


def test_hypersparse_layers(ctx):
    n = 1 << 20
    rows = np.random.default_rng(23).choice(n, 300, replace=False).tolist()
    g = _sparse_graph(n, rows, 24)
    nodes = rows[:40] + [1, 2, n - 1, rows[0] + 1, 12345] + rows[40:60]        # unpopulated rows among them
    check_oracle(g, ["B", "A"], nodes[:8] + [12345, 1])
    check(ctx, g, ["A"], nodes)
    check(ctx, g, ["B", "A"], nodes)
    check(ctx, g, ["B", "A"], nodes, mt_layers=True)


def test_nodes_at_the_top_of_a_wide_id_space(ctx):
    n = 2**32 - 2
    rows = [n - 1, n - 2, n - 70000, 2**31 + 5, 2**31 - 1, 7] + [3 * 10**9 + 977 * j for j in range(40)]
    g = _sparse_graph(n, rows, 31, top=(n - 1, n - 2))
    nodes = [n - 1, n - 2, n - 1, n - 3, n - 70000, 2**31 + 5, 2**31 - 1, 7, 0, 12345] + rows[6:20]
    check_oracle(g, ["A", "B"], nodes[:10])
    # fgpu_expand_edges takes this dimension only where it needs no sort (one type without a dp layer): held to it there
    st = check(ctx, g, ["A", "B"], nodes, expand=False)
    assert st[6] > len(rows), "every populated row points at the two top nodes"
    check(ctx, g, ["A"], nodes)
    check(ctx, g, ["B"], nodes, mt_layers=True, expand=False)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def raw(ctx, nodes, k, m, flags, mt_m=None, multi=None, want=(True, True)):
    """the C call itself, for arguments engine.Context.node_degrees cannot form"""
    from falkordb_amd.engine import _hop_arrays, _p
    ids = np.ascontiguousarray(nodes, dtype=U64) if nodes is not None else None
    size = max(min(k, 70001), 1)                                                 # (a k past that is refused before anything is written)
    o, i = np.full(size, 77, dtype=U64), np.full(size, 77, dtype=U64)
    st = (_ffi.C.c_uint64 * 8)(*([5] * 8))
    code = ctx.lib.fgpu_node_degrees(ctx._h, _p(ids), k, _hop_arrays(m), None, None, _hop_arrays(mt_m) if mt_m else None, None, None,
                                     _hop_arrays(multi) if multi else None, len(m), flags, _p(o) if want[0] else None,
                                     _p(i) if want[1] else None, st)
    _ffi.check(code)
    return o, i, list(st)


def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, lists, plain):
    d = dev(ctx, lists.tensors[0])
    key, off, ids = flat(lists.tensors[0].me)
    partial = ctx.multi_new(key[1:], off[1:] - off[1], ids[int(off[1]):])       # the table lacks the row of (12, 100)
    cases = [
        (lambda: raw(ctx, [5, 6000], 2, [d.m], OUT, multi=[d.multi]), "at or past"),          # an id at n
        (lambda: raw(ctx, [5], 1, [d.m], 0, [d.mt_m], [d.multi]), "flags"),
        (lambda: raw(ctx, [5], 1, [d.m], 4, [d.mt_m], [d.multi]), "flags"),
        (lambda: raw(ctx, [5], 1, [d.m], OUT | IN | 4, [d.mt_m], [d.multi]), "flags"),
        (lambda: raw(ctx, [5], 1, [d.m], IN, None, [d.multi]), "mt_m"),                        # mt_m missing under IN
        (lambda: raw(ctx, [5], 1, [d.m], OUT | IN, None, [d.multi]), "mt_m"),
        (lambda: raw(ctx, [13, 12], 2, [d.m], OUT, multi=[partial]), "no row"),                # a MULTI_EDGE pair without a table row
        (lambda: raw(ctx, [5, 100], 2, [d.m], IN, [d.mt_m], [partial]), "no row"),             # ... met from the far side
        (lambda: raw(ctx, list(range(10)), (1 << 24) + 1, [d.m], OUT), "at most"),
    ]
    ctx.sync()
    for bad, word in cases:
        gc.collect()
        before = ctx.device_bytes()[0]
        seen = []
        with pytest.raises(_ffi.FgpuError) as e:
            seen.append(bad())
        assert e.value.code == _ffi.FGPU_INVALID and word in str(e.value), e.value
        ctx.sync()
        gc.collect()
        assert ctx.device_bytes()[0] == before, "a refused call keeps device memory"
        st = check(ctx, lists, ["T"], [13, 12, 20, 5], expand=False)             # the next call is exact
        assert st[4] == 65
    # an id at n is refused before anything is written, stats are zeroed by every failure
    from falkordb_amd.engine import _hop_arrays, _p
    nodes, o = np.array([5, 6000], dtype=U64), np.full(2, 77, dtype=U64)
    st = (_ffi.C.c_uint64 * 8)(*([5] * 8))
    code = ctx.lib.fgpu_node_degrees(ctx._h, _p(nodes), 2, _hop_arrays([d.m]), None, None, None, None, None, _hop_arrays([d.multi]), 1,
                                     OUT, _p(o), None, st)
    assert code == _ffi.FGPU_INVALID and o.tolist() == [77, 77] and list(st) == [0] * 8
    # out only needs no transposed layer and leaves in_degree alone
    o, i, st = raw(ctx, [16, 13], 2, [d.m], OUT, multi=[d.multi], want=(True, False))
    assert o.tolist() == [5000, 128]
    # without a table on clean layers nothing is read: the pair counts 1 (fgpu.h lets multi be NULL only without MULTI_EDGE)
    p = dev(ctx, plain.tensors[0])
    o, i, st = raw(ctx, [16, 30], 2, [p.m], OUT | IN, [p.mt_m])
    assert o.tolist() == [5000, 1] and i.tolist() == [0, 1] and st[0] == 4


def test_a_call_keeps_no_device_memory(ctx, rnd):
    nodes = list(range(60))
    args = layer_args(ctx, [rnd.tensors[2], rnd.tensors[0]], mt_layers=True)
    call = lambda: ctx.node_degrees(nodes, *args, incoming=True)
    first = call()
    gc.collect()
    ctx.sync()
    before = ctx.device_bytes()[0]
    again = call()
    gc.collect()
    ctx.sync()
    assert ctx.device_bytes()[0] == before
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
