"""fgpu_edges_remove (csrc/edges_remove.hip): a batch of (src, dst, id) triples leaves a tensor's UINT64 base and its transposed
pattern; multi-edge pairs shrink, demote or empty.  The checker is tests/edges_remove_check.py's remove_edges — dicts and
sorted() — every output matrix is read back whole with fgpu_mat_export_csr, and the inputs are checked untouched.  Shapes are the
smallest at which a pass can go wrong: more than one 256-lane workgroup of triples with a partial last one, scans over several
4096-item tiles, one row of m and one multi-edge run longer than a workgroup, a hypersparse input, a non-square matrix."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402
from edges_remove_check import MULTI, remove_edges  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


def split(entries):
    k = sorted(entries)
    return (np.array([r for r, _ in k], dtype=U64), np.array([c for _, c in k], dtype=U64),
            np.array([entries[x] for x in k], dtype=U64))


def build(ctx, nrows, ncols, pairs, hyper=False):
    """(m, mt): the UINT64 matrix of `pairs` — in the hypersparse form when asked — and its BOOL transposed pattern."""
    r, c, v = split(pairs)
    if hyper:
        a = me.build(nrows, ncols, r, c)
        rp, hr = a.hyper()
        m = ctx.mat_from_csr(nrows, ncols, rp, a.colidx, vals=v, hyper_rows=hr)
    else:
        m = ctx.mat_from_coo(nrows, ncols, r, c, v)
    return m, ctx.mat_from_coo(ncols, nrows, c, r)


def flat(rows):
    """The multi-edge rows as the call takes them: keys src << 32 | dst ascending, offsets, ids."""
    keys = sorted(rows)
    off = np.concatenate([[0], np.cumsum([len(rows[k]) for k in keys])]).astype(U64)
    ids = np.array([x for k in keys for x in rows[k]], dtype=U64)
    return np.array([(s << 32) | d for s, d in keys], dtype=U64), off, ids


def assert_matrix(mat, nrows, ncols, kept, valued):
    """mat == the entries `kept`, row by row, through the full export"""
    assert (mat.nrows, mat.ncols, mat.nvals, mat.has_values) == (nrows, ncols, len(kept), valued)
    r, c, v = split(kept)
    rp, ci, vals = mat.export_csr()
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(r.astype(np.int64), minlength=nrows))]).astype(U64))
    assert np.array_equal(ci, c)
    if valued:
        assert vals is not None and np.array_equal(vals, v)
    else:
        assert vals is None


def check(ctx, nrows, ncols, pairs, rows, triples, hyper=False, keep_outputs=False):
    """One call held against remove_edges in everything it returns; returns the stats (and the two outputs when asked)."""
    m, mt = build(ctx, nrows, ncols, pairs, hyper)
    kept, hit, taken, emptied, want_st = remove_edges(pairs, rows, triples)
    t = np.array(triples, dtype=U64).reshape(-1, 3)
    mo, mto, got_hit, got_taken, er, ec, st = engine.edges_remove(ctx, m, mt, t[:, 0], t[:, 1], t[:, 2], *flat(rows), stats=True)
    assert_matrix(mo, nrows, ncols, kept, True)
    assert_matrix(mto, ncols, nrows, {(c, r): 0 for r, c in kept}, False)
    assert got_hit.tolist() == hit
    assert got_taken.tolist() == taken
    assert list(zip(er.tolist(), ec.tolist())) == emptied
    assert st == want_st
    assert_matrix(m, nrows, ncols, pairs, True)                          # the inputs are untouched
    assert_matrix(mt, ncols, nrows, {(c, r): 0 for r, c in pairs}, False)
    return (st, mo, mto) if keep_outputs else st


def multigraph(seed, nrows, count, ncols=None, cols=None):
    """`count` distinct coordinates; every fourth is a multi-edge pair with 2 to 5 ids, the others carry a distinct inline id with
    high bits.  cols: draw the columns from these only.  Returns (pairs, rows)."""
    rng = np.random.default_rng(seed)
    ncols = nrows if ncols is None else ncols
    width = ncols if cols is None else len(cols)
    lin = rng.choice(nrows * width, count, replace=False)
    pairs, rows = {}, {}
    for k, x in enumerate(lin.tolist()):
        key = (x // width, x % width if cols is None else int(cols[x % width]))
        if k % 4 == 0:
            pairs[key] = MULTI
            rows[key] = [(2 << 40) + 8 * k + j for j in range(2 + (k // 4) % 4)]
        else:
            pairs[key] = (1 << 40) + 7 * k
    return pairs, rows


def edges_of(pairs, rows):
    """every stored edge as (src, dst, id), in (src, dst, id) order"""
    return [(s, d, i) for (s, d) in sorted(pairs) for i in (rows[(s, d)] if pairs[(s, d)] == MULTI else [pairs[(s, d)]])]


def mixed_batch(seed, pairs, rows, nrows, ncols, count):
    """`count` triples: three in five name stored edges (drawn with repetition, so some repeat), the others an unknown id on a
    stored pair, an id of another pair, or a pair that is not stored."""
    rng = np.random.default_rng(seed)
    edges = edges_of(pairs, rows)
    out = []
    for k in range(count):
        s, d, i = edges[int(rng.integers(len(edges)))]
        kind = k % 5
        if kind == 3:
            i = edges[int(rng.integers(len(edges)))][2] if k % 2 else 5 + k
        elif kind == 4:
            while (s, d) in pairs:
                s, d = int(rng.integers(nrows)), int(rng.integers(ncols))
        out.append((s, d, i))
    return out


@pytest.fixture(scope="module")
def big():
    return multigraph(5000, 5000, 40000)


def test_a_partial_last_block_of_triples(ctx):
    """300 x 300, 3000 entries, 750 of them multi-edge, 700 triples: three workgroups, the last one of 188 lanes."""
    pairs, rows = multigraph(300, 300, 3000)
    st = check(ctx, 300, 300, pairs, rows, mixed_batch(1, pairs, rows, 300, 300, 700))
    assert st[0] > 300 and st[1] > 0 and st[3] > 0 and st[6] > 100 and st[7] > 100 and 0 < st[4] < 3000


@pytest.mark.parametrize("which", ["none", "one", "all"])
def test_scans_over_several_tiles(ctx, big, which):
    """5000 x 5000, 40 000 entries: the keep scans cross 4096-item tiles, and the 10 000 multi-edge runs hold 35 000 ids.  No
    triple: copies.  Every edge: empty outputs, every pair emptied."""
    pairs, rows = big
    every = edges_of(pairs, rows)
    st = check(ctx, 5000, 5000, pairs, rows, {"none": [], "one": [every[len(every) // 2]], "all": every}[which])
    if which == "none":
        assert st == [0, 0, 0, 0, 40000, 40000, 0, 0]
    if which == "all":
        assert st == [len(every), 40000, 10000, 0, 0, 0, 0, 0]


def test_the_taken_scan_over_several_tiles(ctx, big):
    """Every third id of the 35 000 in the multi-edge runs: runs of 2 demote or stay, longer ones stay, and the scan of taken
    carries counts across its 4096-item tiles.  A second batch takes all but the last id of every run: every pair demotes."""
    pairs, rows = big
    ids = [(s, d, i) for (s, d) in sorted(rows) for i in rows[(s, d)]]
    assert len(ids) > 4096
    st = check(ctx, 5000, 5000, pairs, rows, ids[::3])
    assert st[0] == len(ids[::3]) and st[3] > 0 and st[1] == 0
    st = check(ctx, 5000, 5000, pairs, rows, [(s, d, i) for (s, d) in sorted(rows) for i in rows[(s, d)][:-1]])
    assert st[3] == 10000 and st[1] == 0


def test_a_row_of_m_longer_than_a_workgroup(ctx):
    """Row 777 of a 6000 x 6000 matrix holds 5000 entries; the triples name its first, its last and its middle column, a column
    it does not hold, and entries of the short rows before and after it."""
    n, hub = 6000, 777
    pairs, rows = multigraph(6001, n, 3000)
    cols = np.sort(np.random.default_rng(6000).choice(n, 5000, replace=False)).tolist()
    for k, v in enumerate(cols):
        pairs.setdefault((hub, v), 10**12 + k)
    hubcols = sorted(c for r, c in pairs if r == hub)
    free = next(c for c in range(n) if (hub, c) not in pairs)
    hubs = [(hub, c, pairs[(hub, c)] if pairs[(hub, c)] != MULTI else rows[(hub, c)][0]) for c in
            (hubcols[0], hubcols[-1], hubcols[len(hubcols) // 2], hubcols[1], hubcols[-2])]
    others = [e for e in edges_of(pairs, rows) if e[0] != hub][::97]
    st = check(ctx, n, n, pairs, rows, hubs + [(hub, free, 1)] + others)
    assert st[0] == len(hubs) + len(others) and st[6] == 1


LONG = 5000


def long_run_case():
    pairs, rows = multigraph(77, 300, 600)
    pairs[(150, 150)] = MULTI
    rows[(150, 150)] = [(3 << 40) + 3 * j for j in range(LONG)]
    return pairs, rows


@pytest.mark.parametrize("survivors", [[0], [LONG - 1], [LONG // 2], [], [17, 4000], [0, LONG - 1]],
                         ids=["first", "last", "middle", "none", "two", "both-ends"])
def test_a_multi_edge_run_longer_than_a_workgroup(ctx, survivors):
    """One pair holds 5000 ids.  All but one taken: the pair demotes to the survivor, found without a walk of the run; all taken:
    the pair is emptied; two left: it stays MULTI_EDGE."""
    pairs, rows = long_run_case()
    run = rows[(150, 150)]
    batch = [(150, 150, i) for j, i in enumerate(run) if j not in survivors]
    batch = batch[::-1] + [(150, 150, run[-1] + 1)]                      # any order; one unknown id past the run
    st = check(ctx, 300, 300, pairs, rows, batch)
    assert st[0] == LONG - len(survivors) and st[7] == 1
    assert (st[1], st[2], st[3]) == {0: (1, 1, 0), 1: (0, 0, 1), 2: (0, 0, 0)}[len(survivors)]


def form_of(ctx, mat, nrows):
    """'hyper' or 'full', read off the device memory the snapshot holds: the full form keeps nrows + 1 row pointers — 24 004
    bytes at 6000 rows — and the hypersparse form of these tests (at most 375 stored rows, at most 600 entries) at most
    1.25 x (1536 + 1536 + 2560 + 4864) bytes, the pool's size classes with its quarter of slack, under 14 KiB."""
    ctx.sync()
    before = ctx.device_bytes()[0]
    mat.free()
    ctx.sync()
    held = before - ctx.device_bytes()[0]
    assert held > 0
    return "full" if held >= 4 * (nrows + 1) else "hyper"


def prefer_hyper(nrows, populated):
    return "hyper" if nrows > 4096 and populated * 16 <= nrows else "full"    # fgpu_mat_from_coo's rule (mat.hip)


@pytest.mark.parametrize("case", ["hyper-stays", "full-to-hyper", "stored-hyper-to-full"])
def test_a_hypersparse_input_and_the_form_of_the_outputs(ctx, case):
    """6000 rows.  40 populated rows stored hypersparse stay so; 400 populated rows in the full form of which 120 empty come out
    hypersparse (280 x 16 <= 6000); 400 rows handed in hypersparse of which 10 empty come out in the full form (390 x 16 > 6000).
    The columns come from 30 values, so the transposed pattern is hypersparse throughout."""
    n = 6000
    rng = np.random.default_rng(40)
    populated, per_row, emptying = {"hyper-stays": (40, 10, 5), "full-to-hyper": (400, 1, 120), "stored-hyper-to-full": (400, 1, 10)}[case]
    rws = np.sort(np.r_[rng.choice(np.arange(1, n - 1), populated - 2, replace=False), [0, n - 1]]).tolist()
    cols = rng.choice(n, 30, replace=False)
    pairs, rows = {}, {}
    for a, r in enumerate(rws):
        for b, c in enumerate(rng.choice(cols, per_row, replace=False).tolist()):
            k = a * per_row + b
            if k % 4 == 0:
                pairs[(r, c)] = MULTI
                rows[(r, c)] = [(2 << 40) + 8 * k + j for j in range(2 + k % 3)]
            else:
                pairs[(r, c)] = (1 << 40) + k
    gone_rows = set(rws[1::max(1, populated // emptying)][:emptying - 1] + [rws[-1]])
    batch = [e for e in edges_of(pairs, rows) if e[0] in gone_rows]
    # ... and pieces of the rows that stay, none of which empties a row: the first id of multi-edge pairs, and where a row
    # holds ten pairs some of its single ones
    batch += [(s, d, rows[(s, d)][0]) for s, d in sorted(rows) if s not in gone_rows][::3]
    if per_row > 1:
        batch += [e for e in edges_of(pairs, rows) if e[0] not in gone_rows and pairs[(e[0], e[1])] != MULTI][::9]
    stored_hyper = case != "full-to-hyper"
    st, mo, mto = check(ctx, n, n, pairs, rows, batch, hyper=stored_hyper, keep_outputs=True)
    kept, *_ = remove_edges(pairs, rows, batch)
    left_rows, left_cols = len({r for r, _ in kept}), len({c for _, c in kept})
    assert left_rows == populated - len(gone_rows)
    want = {"hyper-stays": "hyper", "full-to-hyper": "hyper", "stored-hyper-to-full": "full"}[case]
    assert prefer_hyper(n, left_rows) == want and prefer_hyper(n, left_cols) == "hyper"
    assert form_of(ctx, mo, n) == want
    assert form_of(ctx, mto, n) == "hyper"


def test_a_rectangular_matrix(ctx):
    """300 x 500: the transposed pattern is searched by column ids past the row dimension."""
    pairs, rows = multigraph(500, 300, 3000, ncols=500)
    assert max(c for _, c in pairs) >= 300
    st = check(ctx, 300, 500, pairs, rows, mixed_batch(2, pairs, rows, 300, 500, 900))
    assert st[0] > 0 and st[1] > 0 and st[3] > 0


def test_duplicates_and_unknowns_in_one_batch(ctx):
    pairs, rows = multigraph(301, 300, 2000)
    edges = edges_of(pairs, rows)
    s, d = next(k for k in sorted(rows) if len(rows[k]) >= 3)
    r = rows[(s, d)]
    single = next(e for e in edges if pairs[(e[0], e[1])] != MULTI)
    other = next(k for k in sorted(rows) if k != (s, d))
    batch = [(s, d, r[0]), single, (s, d, r[0]), (s, d, rows[other][0]), (s, d, 7), single, (single[0], single[1], 7),
             (other[0], other[1], single[2]), (s, d, r[1]), (s, d, r[1])]
    st = check(ctx, 300, 300, pairs, rows, batch)
    assert st[0] == 6 and st[1] == 1 and st[7] == 4 and st[3] == (1 if len(r) == 3 else 0)
    m, mt = build(ctx, 300, 300, pairs)
    t = np.array(batch, dtype=U64)
    a = engine.edges_remove(ctx, m, mt, t[:, 0], t[:, 1], t[:, 2], *flat(rows), stats=True)
    p = np.random.default_rng(9).permutation(len(batch))                  # the order of the batch does not matter
    b = engine.edges_remove(ctx, m, mt, t[p, 0], t[p, 1], t[p, 2], *flat(rows), stats=True)
    plain = lambda res: ([x.tolist() for x in res[0].export_csr()], [x.tolist() for x in res[1].export_csr()[:2]],
                         res[3].tolist(), res[4].tolist(), res[5].tolist(), res[6])
    assert plain(a) == plain(b) and b[2].tolist() == a[2][p].tolist()
    mo, mto, hit, taken, er, ec = engine.edges_remove(ctx, m, mt, t[:, 0], t[:, 1], t[:, 2], *flat(rows), want_hit=False)
    assert hit is None and taken.tolist() == a[3].tolist()


def _raises_invalid(fn):
    with pytest.raises(_ffi.FgpuError) as e:
        fn()
    assert e.value.code == _ffi.FGPU_INVALID
    assert str(e.value).split(":", 1)[1].strip()   # fgpu_last_error is set


def test_rejections_leave_the_context_usable(ctx):
    pairs, rows = multigraph(303, 300, 2000)
    m, mt = build(ctx, 300, 300, pairs)
    rpairs, rrows = multigraph(67, 300, 500, ncols=64)
    rect, rect_t = build(ctx, 300, 64, rpairs)
    boolean = ctx.mat_from_coo(300, 300, [1], [2])
    valued_t = ctx.mat_from_coo(300, 300, [1], [2], [3])
    key, off, ids = flat(rows)
    (s, d), run = next(iter(sorted(rows.items())))
    e = next(x for x in edges_of(pairs, rows) if pairs[(x[0], x[1])] != MULTI)
    call = lambda mm, tt, ss, dd, ii, k=key, o=off, i=ids: engine.edges_remove(ctx, mm, tt, ss, dd, ii, k, o, i)
    swapped = ids.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    equal = ids.copy()
    equal[1] = equal[0]
    short = off.copy()
    short[1:] -= off[1] - U64(1)                                          # the first run keeps one id
    short_ids = np.r_[ids[:1], ids[int(off[1]):]]
    marker = ids.copy()
    marker[int(off[1]) - 1] = MULTI
    cases = [
        lambda: call(m, mt, [300], [0], [1]),                             # a source at its dimension
        lambda: call(m, mt, [0], [2**40], [1]),                           # a destination past it
        lambda: call(rect, rect_t, [5], [64], [1], *flat(rrows)),         # ... at the COLUMN dimension of a non-square matrix
        lambda: call(m, mt, [e[0], 1], [e[1], 1], [e[2], MULTI]),         # the marker as an id
        lambda: call(boolean, mt, [1], [2], [1]),                         # m not valued
        lambda: call(m, None, [1], [2], [1]),                             # mt missing
        lambda: call(m, valued_t, [1], [2], [1]),                         # mt valued
        lambda: call(m, rect_t, [1], [2], [1]),                           # mt of other dimensions
        lambda: call(m, mt, [1], [2], [1], key[::-1].copy()),             # keys descending
        lambda: call(m, mt, [1], [2], [1], np.r_[key[:1], key[:-1]]),     # a key twice
        lambda: call(m, mt, [1], [2], [1], key, short, short_ids),        # a run shorter than 2
        lambda: call(m, mt, [1], [2], [1], key, off, swapped),            # ids descending in a run
        lambda: call(m, mt, [1], [2], [1], key, off, equal),              # ... or repeated
        lambda: call(m, mt, [1], [2], [1], key, off, marker),             # the marker as the last id of a run
        lambda: call(m, mt, [e[0], s], [e[1], d], [e[2], run[0]], key[1:], off[1:] - off[1], ids[int(off[1]):]),   # no row for (s, d)
        lambda: call(m, mt, [s], [d], [5], [], [0], []),                  # ... even when the id would be unknown
    ]
    ctx.sync()
    for bad in cases:
        before = ctx.device_bytes()[0]
        _raises_invalid(bad)
        ctx.sync()
        assert ctx.device_bytes()[0] == before, "a rejected call keeps device memory"
        check(ctx, 300, 300, pairs, rows, [e, (s, d, run[0])])            # the next call is exact
    # a key m does not hold is ignored
    call(m, mt, [s], [d], [5], np.r_[key, [U64(2**63)]], np.r_[off, [off[-1] + U64(2)]], np.r_[ids, np.array([1, 2], dtype=U64)])


def test_too_many_triples_is_rejected_before_the_arrays_are_read(ctx):
    """n >= 2^32 - 1: the count alone is refused (the arrays behind it are never touched, so one element stands in)."""
    pairs, rows = multigraph(305, 300, 500)
    m, mt = build(ctx, 300, 300, pairs)
    one = np.zeros(1, dtype=np.uint64)
    p = one.ctypes.data_as(_ffi.u64p)
    mo, mto = C.c_void_p(), C.c_void_p()
    er, ec = _ffi.u64p(), _ffi.u64p()
    ne = C.c_uint64()
    for n in (2**32 - 1, 2**32):
        code = ctx.lib.fgpu_edges_remove(ctx.handle, m._h, mt._h, p, p, p, C.c_uint64(n), None, p, None, C.c_uint64(0), C.byref(mo),
                                         C.byref(mto), None, None, C.byref(er), C.byref(ec), C.byref(ne), None)
        assert code == _ffi.FGPU_INVALID and ctx.lib.fgpu_last_error()
        assert not mo.value and not mto.value and not er and not ec and ne.value == 0
    check(ctx, 300, 300, pairs, rows, edges_of(pairs, rows)[::50])


def test_a_call_keeps_no_device_memory(ctx):
    """As tests/test_gpu_nodes_detach.py: warm, read in_use, call again, free what came back — in_use is where it was."""
    pairs, rows = multigraph(304, 5000, 20000)
    m, mt = build(ctx, 5000, 5000, pairs)
    t = np.array(edges_of(pairs, rows)[::3], dtype=U64)
    fl = flat(rows)

    def call():
        res = engine.edges_remove(ctx, m, mt, t[:, 0], t[:, 1], t[:, 2], *fl, stats=True)
        plain = (res[0].nvals, res[1].nvals, res[2].tolist(), res[3].tolist(), res[4].tolist(), res[5].tolist(), res[6])
        res[0].free()
        res[1].free()
        del res
        gc.collect()
        return plain
    first = call()
    ctx.sync()
    in_use = ctx.device_bytes()[0]
    second = call()
    ctx.sync()
    assert ctx.device_bytes()[0] == in_use and second == first
