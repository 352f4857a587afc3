"""fgpu_expand_edges / fgpu_multi (csrc/expand_edges.hip): CondTraverse's per-row path for a whole batch, the relationship
emitted.  The expected value is always oracle.model.expand_row, called row by row over the same tensors, the rows concatenated
with the row index in front; all four columns are compared for equality.  Shapes are the smallest at which a pass can go wrong:
rows of 0, 1 and 70 entries, a row and an id list past one workgroup (and past the 64 / 4096 sizes of the engine's sorters), an
output past 2^20 ids (the placement scan crosses its blocks), hypersparse layers, 70 000 rows."""
import gc

import numpy as np
import pytest

from falkordb_amd import _ffi, host

from oracle import model

pytestmark = pytest.mark.gpu
U64 = np.uint64
MULTI = model.MULTI_EDGE


# ---- the oracle's tensors on the device ------------------------------------------------------------------------------
def _coo(ctx, n, entries, valued):
    """entries: {(r, c): v} or a set of (r, c) -> a device matrix, None when there is nothing to store"""
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


_DEV = {}


def dev(ctx, T, mt_layers=False):
    key = (id(T), mt_layers)
    if key not in _DEV:
        _DEV[key] = (T, Dev(ctx, T, mt_layers))   # (the tensor is kept: its id stays its own)
    return _DEV[key][1]


def bitmap(g, labels):
    lids = [g.label_ids[l] for l in labels]
    words = np.zeros((g.n + 63) // 64, dtype=U64)
    for v in range(g.n):
        if all((v, l) in g.node_labels for l in lids):
            words[v >> 6] |= U64(1) << U64(v & 63)
    return words


def want_rows(g, froms, tos, types, **kw):
    """expand_row per row (one oracle call per DISTINCT (from, to): the rows of a batch repeat), as an (N, 4) array"""
    memo, out = {}, []
    kw.setdefault("emit_relationship", True)              # (the default of got_rows)
    for i, (f, t) in enumerate(zip(froms, tos)):
        if f is None and t is None:
            continue                                      # the raw call skips the full-matrix walk
        if (f, t) not in memo:
            memo[(f, t)] = np.array(model.expand_row(g, f, t, types, **kw), dtype=U64).reshape(-1, 3)
        a = memo[(f, t)]
        out.append(np.concatenate([np.full((len(a), 1), i, dtype=U64), a], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), dtype=U64)


def got_rows(ctx, g, froms, tos, types, mt_layers=False, transposed=False, bidirectional=False, emit_relationship=True,
             from_labels=(), to_labels=(), with_mt=True):
    scan = [g.type_ids[t] for t in types] if types else list(range(len(g.tensors)))
    d = [dev(ctx, g.tensors[t], mt_layers) for t in scan]
    res = ctx.expand_edges(froms, tos, [x.m for x in d], [x.dp for x in d], [x.dm for x in d],
                           [x.mt_m for x in d] if with_mt else None, [x.mt_dp for x in d] if with_mt else None,
                           [x.mt_dm for x in d] if with_mt else None, [x.multi for x in d], transposed=transposed,
                           bidirectional=bidirectional, first_only=not emit_relationship,
                           from_bitmap=bitmap(g, from_labels) if from_labels else None,
                           to_bitmap=bitmap(g, to_labels) if to_labels else None)
    row, f, t, e, st = res
    return np.stack([row.astype(U64), f.astype(U64), t.astype(U64), e], axis=1), st


def check(ctx, g, froms, tos, types, mt_layers=False, **kw):
    got, st = got_rows(ctx, g, froms, tos, types, mt_layers, **kw)
    want = want_rows(g, froms, tos, types, **kw)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert st[2] == len(want)
    return st


# ---- graphs ------------------------------------------------------------------------------------------------------------
def single_type(n, pairs, me=None, dp=None, dm=None):
    g = model.Graph(n)
    g.add_type("T")
    g.tensors[0] = model.Tensor(n, n, m=pairs, dp=dp, dm=dm, me=me)
    g.adjacency.m = g.tensors[0].structure()
    return g


@pytest.fixture(scope="module")
def clean():
    """rows of 0 (node 5), 1 (node 6) and 70 entries (node 7, every 10th pair multi-edge), and a few other rows"""
    pairs, me = {(6, 2999): 600}, {}
    for j in range(70):
        pairs[(7, 3 + 41 * j)] = 7000 + j
        if j % 10 == 3:
            pairs[(7, 3 + 41 * j)] = MULTI
            me[(7, 3 + 41 * j)] = [90000 + 100 * j + x for x in range(2 + j % 3)]
    for v in range(100, 140):
        pairs[(v, (v * 37) % 3000)] = 100000 + v
        pairs[(v, 7)] = 200000 + v
    return single_type(3000, pairs, me)


@pytest.fixture(scope="module")
def dirty():
    """one type whose deltas are not folded: a dp entry shadowing an m entry with another id, a dp-only pair, a dm tombstone,
    a multi-edge pair in dp, a tombstoned pair that dp re-adds, and a self-loop"""
    m = {(1, 2): 10, (1, 3): 11, (1, 4): MULTI, (2, 5): 12, (1, 9): 13, (8, 1): 14, (9, 1): 15, (1, 1): 16, (4, 12): 17}
    dp = {(1, 2): 20, (1, 6): 21, (1, 7): MULTI, (7, 1): 22, (4, 12): 23, (11, 1): MULTI}
    dm = {(1, 3), (9, 1), (4, 12)}
    me = {(1, 4): [40, 41], (1, 7): [30, 31, 32], (11, 1): [50, 51]}
    return single_type(64, m, me, dp, dm)


def random_graph(seed, n, npairs, ntypes=3, loops=8, labels=True):
    """ntypes tensors over shared pairs (so that one pair sits in several), a quarter of the pairs multi-edge, every tensor
    with unfolded deltas of all four kinds, some self-loops, two labels"""
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
            kind = int(rng.integers(0, 10))
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
    if labels:
        for name, mod in (("P", 3), ("Q", 2)):
            lid = g.add_label(name)
            g.node_labels |= {(v, lid) for v in range(n) if (v * 7 + lid) % mod == 0}
    return g


@pytest.fixture(scope="module")
def rnd():
    return random_graph(11, 60, 260)


# ---- single type -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 1024])
def test_clean_single_type(ctx, clean, k):
    froms = [7] if k == 1 else [(5, 6, 7, 7, 100 + i % 40, 2000)[i % 6] for i in range(k)]   # 7 twice in a row: a duplicated source
    st = check(ctx, clean, froms, [None] * k, ["T"])
    assert st[5] == 0, "one type without a dp layer is ordered by the entry positions"
    assert st[1] == 0 and st[3] > 0 and st[4] == 4
    st = check(ctx, clean, froms, [None] * k, ["T"], emit_relationship=False)
    assert st[5] == 0 and st[4] == 1


@pytest.mark.parametrize("mt_layers", [False, True])
def test_dirty_single_type(ctx, dirty, mt_layers):
    nodes = list(range(13))
    for kw in (dict(), dict(emit_relationship=False), dict(bidirectional=True), dict(transposed=True),
               dict(bidirectional=True, transposed=True, emit_relationship=False)):
        st = check(ctx, dirty, nodes, [None] * 13, ["T"], mt_layers, **kw)
        assert st[5] >= 1
        check(ctx, dirty, [None] * 13, nodes, ["T"], mt_layers, **kw)
        check(ctx, dirty, [1, 1, 1, 4, 1, 7, 1], [2, 3, 7, 12, 1, 1, 6], ["T"], mt_layers, **kw)


# ---- past one workgroup, past the sorters, past one scan block --------------------------------------------------------
def test_hub_row_long_list_and_large_output(ctx):
    n = 6000
    pairs = {(17, c): 500000 + c for c in range(0, 5000)}                  # a hub row of 5000 entries
    pairs[(17, 5500)] = MULTI
    pairs[(18, 3)] = MULTI
    pairs[(19, 4)] = MULTI
    pairs[(4, 19)] = 77
    me = {(17, 5500): [9, 10], (18, 3): list(range(10**6, 10**6 + 5000)),   # a 5000-id list
          (19, 4): list(range(2 * 10**6, 2 * 10**6 + 3 * 70000, 3))}        # a 70 000-id list
    g = single_type(n, pairs, me)
    st = check(ctx, g, [17, 18, 16, 17], [None] * 4, ["T"])
    assert st[0] == 2 * 5001 + 1 and st[4] == 5000
    check(ctx, g, [None, None], [3, 4000], ["T"])                          # ... and walked from the far side
    st = check(ctx, g, [19] * 16, [None] * 16, ["T"], bidirectional=True)   # 16 x 70 000 ids; the reverse pass adds (4, 19), (17, 19)
    assert st[2] == 16 * 70002 > 2**20 and st[4] == 70000
    st = check(ctx, g, [19] * 16, [None] * 16, ["T"], emit_relationship=False)
    assert st[2] == 16


# ---- several types -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emit", [True, False])
@pytest.mark.parametrize("mt_layers", [False, True])
def test_three_types_in_scan_order(ctx, rnd, emit, mt_layers):
    """C, A, B: not ascending.  The pairs are shared, so many sit in two or three types, multi-edge in one"""
    g = rnd
    shared = [p for p in g.tensors[0].structure() if p in g.tensors[2].structure()]
    assert shared and any(g.tensors[0].eff_get(*p) == MULTI or g.tensors[2].eff_get(*p) == MULTI for p in shared)
    nodes = list(range(60))
    for types in (["C", "A", "B"], ["B", "A"], ["C"]):
        st = check(ctx, g, nodes, [None] * 60, types, mt_layers, emit_relationship=emit)
        assert st[5] == 1
        check(ctx, g, [None] * 60, nodes, types, mt_layers, emit_relationship=emit, bidirectional=True)


def test_no_types_on_a_graph_built_through_create_edges():
    """No type named: the reference walks the adjacency, the device the union of the tensors' structures — the same pairs as
    long as every writer keeps the adjacency that union.  Held here on a host-layer Graph written through create_edges, a
    delete and a commit, against the oracle over the same edges."""
    hctx = host.Context(0)
    n = 50
    rng = np.random.default_rng(5)
    g, og = host.Graph(hctx, n), model.Graph(n)
    per_type, eid = [{}, {}, {}], 0
    for t, name in enumerate("XYZ"):
        tid = g.add_type(name)
        og.add_type(name)
        for rnd_ in range(2):
            s, d = rng.integers(0, n, 120), rng.integers(0, n, 120)
            ids = np.arange(eid, eid + 120)
            eid += 120
            g.create_edges(tid, s, d, ids)
            for a, b, e in zip(s.tolist(), d.tolist(), ids.tolist()):
                per_type[t].setdefault((a, b), []).append(e)
            if rnd_ == 0:
                g.commit()
        for p in list(per_type[t])[:15]:
            for e in per_type[t].pop(p):
                g.delete_edge(tid, p[0], p[1], e)
        og.tensors[t] = model.Tensor(n, n, m={p: (es[0] if len(es) == 1 else MULTI) for p, es in per_type[t].items()},
                                     me={p: es for p, es in per_type[t].items() if len(es) > 1})
    og.adjacency.m = set().union(*[set(p) for p in per_type])
    nodes = list(range(n))
    for emit, bidir in ((True, False), (False, True), (True, True)):
        spec = host.cond_spec(hops=[([], [])], emit=emit, bidir=bidir)
        for froms, tos in ((nodes, [None] * n), ([None] * n, nodes)):
            rows, nulls, st = g.cond_traverse_edges_batch(spec, froms, tos)
            want = want_rows(og, froms, tos, [], emit_relationship=emit, bidirectional=bidir)
            assert np.array_equal(np.array(rows, dtype=U64).reshape(-1, 4), want)
            assert nulls == [] and st[5] >= 1
    del g
    gc.collect()
    hctx.close()


# ---- direction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt_layers", [False, True])
@pytest.mark.parametrize("emit", [True, False])
def test_directions(ctx, rnd, mt_layers, emit):
    g = rnd
    nodes = list(range(60))
    loops = [s for s, d in g.adjacency.m if s == d]
    assert loops
    some_to = [(v * 13) % 60 if v % 3 == 0 else None for v in nodes]           # `to` pre-bound on some rows
    pairs = sorted(g.adjacency.m)[:60]
    for types in (["A"], ["B", "C", "A"]):
        for transposed, bidir in ((True, False), (False, True), (True, True)):
            kw = dict(transposed=transposed, bidirectional=bidir, emit_relationship=emit)
            check(ctx, g, nodes, [None] * 60, types, mt_layers, **kw)          # in-only when transposed
            check(ctx, g, [None] * 60, nodes, types, mt_layers, **kw)
            check(ctx, g, nodes, some_to, types, mt_layers, **kw)
            check(ctx, g, [p[0] for p in pairs] + loops, [p[1] for p in pairs] + loops, types, mt_layers, **kw)   # both bound
            check(ctx, g, [p[1] for p in pairs], [p[0] for p in pairs], types, mt_layers, **kw)
    # a self-loop comes out once under a bidirectional pattern: from the forward pass only
    v = loops[0]
    got, _ = got_rows(ctx, g, [v], [v], [], bidirectional=True)
    ids = [e for t in g.tensors for e in t.get(v, v)]
    assert got[:, 3].tolist() == ids


def test_an_out_only_batch_needs_no_transposed_layers(ctx, rnd):
    nodes = list(range(60))
    got, _ = got_rows(ctx, rnd, nodes, [None] * 60, ["A", "B"], with_mt=False)
    assert np.array_equal(got, want_rows(rnd, nodes, [None] * 60, ["A", "B"]))


# ---- labels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [dict(from_labels=["P"]), dict(to_labels=["Q"]), dict(from_labels=["Q"], to_labels=["P"]),
                                    dict(from_labels=["P", "Q"], to_labels=["Q"])], ids=str)
def test_label_bitmaps(ctx, rnd, labels):
    nodes = list(range(60))
    for transposed, bidir in ((False, False), (True, False), (False, True), (True, True)):
        kw = dict(transposed=transposed, bidirectional=bidir, **labels)
        check(ctx, rnd, nodes, [None] * 60, ["B", "A"], **kw)
        check(ctx, rnd, [None] * 60, nodes, [], **kw)


# ---- hypersparse layers, many rows -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse():
    """n = 2^20 with 300 populated rows (what fgpu_mat_from_coo stores hypersparse), two types, a dp layer in one"""
    n = 1 << 20
    rng = np.random.default_rng(23)
    rows = rng.choice(n, 300, replace=False)
    g = model.Graph(n)
    eid = 5
    for t in range(2):
        g.add_type("AB"[t])
        m, dp, dm, me = {}, {}, set(), {}
        for r in rows.tolist():
            for c in rng.choice(n, int(rng.integers(1, 6)), replace=False).tolist() + [int(rows[0])]:
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
    return g, rows.tolist()


def test_hypersparse_layers(ctx, sparse):
    g, rows = sparse
    assert dev(ctx, g.tensors[0]).m.nvals == len(g.tensors[0].m)
    froms = rows[:40] + [1, 2, (1 << 20) - 1, rows[0] + 1] + rows[40:60]       # unpopulated rows among them
    st = check(ctx, g, froms, [None] * len(froms), ["A"])
    assert st[5] == 0
    st = check(ctx, g, froms, [None] * len(froms), ["B", "A"], bidirectional=True)
    assert st[5] == 2, "the key space (row, pass, node) is past one sort: two stable sorts"
    check(ctx, g, [None] * len(froms), froms, ["B", "A"], mt_layers=True)
    check(ctx, g, [None] * 3, [rows[0], 12345, 7], ["A", "B"], emit_relationship=False)


def test_seventy_thousand_rows(ctx, clean):
    """past 16-bit row indices; the sources cycle through a few nodes"""
    k = 70000
    froms = [(7, 5, 6, 101, 2000)[i % 5] for i in range(k)]
    check(ctx, clean, froms, [None] * k, ["T"])
    tos = [(7, 2999, 5)[i % 3] for i in range(k)]
    check(ctx, clean, [None] * k, tos, ["T"], bidirectional=True)


def test_empty_inputs(ctx, clean):
    got, st = got_rows(ctx, clean, [], [], ["T"])
    assert got.shape == (0, 4) and st[2] == 0
    row, f, t, e, st = ctx.expand_edges([7], [None], [])
    assert len(row) == len(f) == len(t) == len(e) == 0
    got, st = got_rows(ctx, clean, [None, 5], [None, None], ["T"])              # nothing bound, and a row without entries
    assert got.shape == (0, 4)


# ---- errors ------------------------------------------------------------------------------------------------------------
def _raises_invalid(fn):
    with pytest.raises(_ffi.FgpuError) as e:
        fn()
    assert e.value.code == _ffi.FGPU_INVALID, e.value
    assert str(e.value)


def test_rejected_calls_keep_nothing_and_leave_the_context_usable(ctx, clean, dirty):
    d = dev(ctx, clean.tensors[0])
    small = dev(ctx, dirty.tensors[0])
    boolean = ctx.mat_from_coo(3000, 3000, [1], [2])
    key, off, ids = flat(clean.tensors[0].me)
    partial = ctx.multi_new(key[1:], off[1:] - off[1], ids[int(off[1]):])       # the table lacks its first row
    call = lambda f, t, m=d.m, mt=d.mt_m, mu=d.multi, **kw: ctx.expand_edges(f, t, [m], None, None, [mt] if mt else None, None, None,
                                                                            [mu], **kw)
    swapped = ids.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    short = off.copy()
    short[1:] -= off[1] - U64(1)
    marker = ids.copy()
    marker[int(off[1]) - 1] = MULTI
    cases = [
        lambda: call([3000], [None]),                                          # a bound id at the dimension
        lambda: call([None], [2**40]),                                         # ... and past it
        lambda: call([7], [None], mu=partial),                                 # a MULTI_EDGE pair with no table row
        lambda: call([7], [None], mu=None),                                    # ... with no table at all
        lambda: call([None], [7], mt=None),                                    # an in-walk without mt
        lambda: call([7], [None], mt=None, transposed=True),
        lambda: call([7], [None], mt=None, bidirectional=True),
        lambda: call([7], [None], m=boolean),                                  # an unvalued m
        lambda: call([7], [None], m=small.m),                                  # layers of differing dimensions
        lambda: call([7], [None], mt=small.mt_m, bidirectional=True),
        lambda: ctx.expand_edges([7], [None], [d.m] * 65),                     # too many types
        lambda: ctx.multi_new(key[::-1].copy(), off, ids),                     # keys descending
        lambda: ctx.multi_new(np.r_[key[:1], key[:-1]], off, ids),             # a key twice
        lambda: ctx.multi_new(key, off + U64(1), np.r_[ids, ids[:1]]),         # off[0] != 0
        lambda: ctx.multi_new(key, short, np.r_[ids[:1], ids[int(off[1]):]]),  # a run shorter than 2
        lambda: ctx.multi_new(key, off, swapped),                              # ids descending in a run
        lambda: ctx.multi_new(key, off, np.r_[ids[:1], ids[:1], ids[2:]]),     # ... or repeated
        lambda: ctx.multi_new(key, off, marker),                               # the marker as an id
    ]
    ctx.sync()
    for bad in cases:
        gc.collect()
        before = ctx.device_bytes()[0]
        _raises_invalid(bad)
        ctx.sync()
        gc.collect()
        assert ctx.device_bytes()[0] == before, "a rejected call keeps device memory"
        check(ctx, clean, [7, 6], [None, None], ["T"])                         # the next call is exact
    assert d.multi.size() == (len(key), len(ids))
    assert ctx.multi_new([], [0], []).size() == (0, 0)


def test_a_call_keeps_no_device_memory(ctx, rnd):
    nodes = list(range(60))
    call = lambda: got_rows(ctx, rnd, nodes, [None] * 60, ["C", "A", "B"], bidirectional=True)[0].copy()
    first = call()
    gc.collect()
    ctx.sync()
    before = ctx.device_bytes()[0]
    again = call()
    gc.collect()
    ctx.sync()
    assert ctx.device_bytes()[0] == before
    assert np.array_equal(first, again)
