"""fgpu_edges_union (csrc/edges_union.hip): one built batch joins a tensor's UINT64 base and its transposed pattern; a pair both
hold is promoted or extended, its ids merged.  The checker is tests/edges_union_check.py's union_edges — dicts and sorted() —
every output matrix is read back whole with fgpu_mat_export_csr, and the inputs are checked untouched.  Shapes are the smallest at
which a pass can go wrong: more than one 256-lane workgroup of batch entries with a partial last one, scans over several 4096-item
tiles, one row of m and runs on either side longer than a workgroup, the hypersparse forms, a non-square matrix."""
import gc
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402
from edges_union_check import MULTI, build_edges, union_edges  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


def split(entries):
    k = sorted(entries)
    return (np.array([r for r, _ in k], dtype=U64), np.array([c for _, c in k], dtype=U64),
            np.array([entries[x] for x in k], dtype=U64))


def build(ctx, nrows, ncols, pairs, hyper=False):
    """(m, mt): the UINT64 matrix of `pairs` — in the hypersparse form when asked — and its BOOL transposed pattern."""
    if not pairs:
        return engine.edges_build(ctx, nrows, ncols, [], [], [])[:2]
    r, c, v = split(pairs)
    if hyper:
        a = me.build(nrows, ncols, r, c)
        rp, hr = a.hyper()
        m = ctx.mat_from_csr(nrows, ncols, rp, a.colidx, vals=v, hyper_rows=hr)
    else:
        m = ctx.mat_from_coo(nrows, ncols, r, c, v)
    return m, ctx.mat_from_coo(ncols, nrows, c, r)


def flat(rows):
    """Multi-edge rows as the call takes and returns them: keys src << 32 | dst ascending, offsets, ids."""
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


def transposed(pairs):
    return {(c, r): 0 for r, c in pairs}


def check(ctx, nrows, ncols, pairs, rows, bpairs, brows, hyper=False, bhyper=False, keep_outputs=False):
    """One call held against union_edges in everything it returns; returns the stats (and the two outputs when asked)."""
    m, mt = build(ctx, nrows, ncols, pairs, hyper)
    fwd, bwd = build(ctx, nrows, ncols, bpairs, bhyper)
    merged, out, want_st = union_edges(pairs, rows, bpairs, brows)
    mo, mto, ok, oo, oi, st = engine.edges_union(ctx, m, mt, *flat(rows), fwd, bwd, *flat(brows), stats=True)
    assert_matrix(mo, nrows, ncols, merged, True)
    assert_matrix(mto, ncols, nrows, transposed(merged), False)
    wk, wo, wi = flat(out)
    assert np.array_equal(ok, wk) and np.array_equal(oo, wo) and np.array_equal(oi, wi)
    assert st == want_st and len(ok) == st[1]
    assert_matrix(m, nrows, ncols, pairs, True)                          # the inputs are untouched
    assert_matrix(mt, ncols, nrows, transposed(pairs), False)
    assert_matrix(fwd, nrows, ncols, bpairs, True)
    assert_matrix(bwd, ncols, nrows, transposed(bpairs), False)
    return (st, mo, mto) if keep_outputs else st


def multigraph(seed, nrows, count, ncols=None):
    """`count` distinct coordinates; every fourth is a multi-edge pair with 2 to 5 ids, the others carry a distinct inline id with
    high bits.  Returns (pairs, rows)."""
    rng = np.random.default_rng(seed)
    ncols = nrows if ncols is None else ncols
    lin = rng.choice(nrows * ncols, count, replace=False)
    pairs, rows = {}, {}
    for k, x in enumerate(lin.tolist()):
        key = (x // ncols, x % ncols)
        if k % 4 == 0:
            pairs[key] = MULTI
            rows[key] = [(2 << 40) + 8 * k + j for j in range(2 + (k // 4) % 4)]
        else:
            pairs[key] = (1 << 40) + 7 * k
    return pairs, rows


def dress(keys):
    """A batch on `keys` in the order given: every fourth a multi-edge pair with 2 to 5 ids, the others one id — ids no
    multigraph() holds, some below and some above the ids it does."""
    bpairs, brows = {}, {}
    for k, key in enumerate(keys):
        base = (5 << 40) if k % 2 else (1 << 30)
        if k % 4 == 0:
            bpairs[key] = MULTI
            brows[key] = [base + 8 * k + j for j in range(2 + (k // 4) % 4)]
        else:
            bpairs[key] = base + 7 * k
    return bpairs, brows


def batch_on(seed, pairs, nrows, ncols, count, colliding):
    """`count` pairs, `colliding` of them stored in `pairs` and the others not, in a shuffled order."""
    rng = np.random.default_rng(seed)
    stored = sorted(pairs)
    keys = [stored[i] for i in rng.choice(len(stored), colliding, replace=False).tolist()]
    fresh = set()
    while len(fresh) < count - colliding:
        key = (int(rng.integers(nrows)), int(rng.integers(ncols)))
        if key not in pairs:
            fresh.add(key)
    keys += sorted(fresh)
    return dress([keys[i] for i in rng.permutation(len(keys)).tolist()])


@pytest.fixture(scope="module")
def big():
    return multigraph(5000, 5000, 40000)


def test_a_partial_last_block_of_batch_entries(ctx):
    """300 x 300, 3000 entries, 750 of them multi-edge; 700 pairs in fwd: three workgroups, the last one of 188 lanes.  Half
    collide, a quarter of the batch's pairs are multi-edge."""
    pairs, rows = multigraph(300, 300, 3000)
    bpairs, brows = batch_on(1, pairs, 300, 300, 700, 350)
    assert len(brows) == 175
    st = check(ctx, 300, 300, pairs, rows, bpairs, brows)
    assert st[0] == 350 and st[1] == 350 and st[2] > 200 and st[3] > 50 and st[4] > 1000 and 4 <= st[5] <= 10


@pytest.mark.parametrize("which", ["empty", "disjoint", "all", "one"])
def test_scans_over_several_tiles(ctx, big, which):
    """5000 x 5000, 40 000 entries: the scans of fwd's flags and the shift of m's entries cross 4096-item tiles.  An empty batch:
    copies.  12 000 pairs m does not hold: nothing collides.  Exactly m's pairs: everything does, 40 000 out rows."""
    pairs, rows = big
    if which == "empty":
        bpairs, brows = {}, {}
    elif which == "disjoint":
        bpairs, brows = batch_on(2, pairs, 5000, 5000, 12000, 0)
    elif which == "all":
        bpairs, brows = dress(sorted(pairs))
    else:
        bpairs, brows = {sorted(pairs)[20001]: 12345}, {}
    st = check(ctx, 5000, 5000, pairs, rows, bpairs, brows)
    if which == "empty":
        assert st == [0, 0, 0, 0, 0, 0, 40000, 40000]
    if which == "disjoint":
        assert st == [12000, 0, 0, 0, 0, 0, 52000, 52000]
    if which == "all":
        assert st[:4] == [0, 40000, 30000, 10000] and st[4] > 100000 and st[6:] == [40000, 40000]
    if which == "one":
        assert st[:2] == [0, 1] and st[4] == st[5] and st[6] == 40000


def test_a_row_of_m_longer_than_a_workgroup(ctx):
    """Row 777 of a 6000 x 6000 matrix holds 5000 entries between columns 10 and 5989; the batch names its first, its last and
    its middle stored column, new columns before the first, between two stored ones and past the last, and stored and new pairs
    of the short rows around it."""
    n, hub = 6000, 777
    pairs, rows = multigraph(6001, n, 3000)
    pairs = {k: v for k, v in pairs.items() if k[0] != hub}
    rows = {k: v for k, v in rows.items() if k[0] != hub}
    cols = np.sort(np.random.default_rng(6000).choice(np.arange(10, n - 10), 5000, replace=False)).tolist()
    for k, c in enumerate(cols):
        if k % 4 == 0:
            pairs[(hub, c)] = MULTI
            rows[(hub, c)] = [10**13 + 4 * k, 10**13 + 4 * k + 2]
        else:
            pairs[(hub, c)] = 10**12 + k
    gap = next(c for c in range(cols[0], cols[-1]) if (hub, c) not in pairs)
    keys = [(hub, c) for c in (cols[0], cols[-1], cols[len(cols) // 2], cols[1], cols[-2], 0, 9, gap, n - 10, n - 1)]
    keys += [k for k in sorted(pairs) if k[0] != hub][::97]
    keys += [(r, c) for r in (hub - 1, hub + 1) for c in (0, 3000, n - 1) if (r, c) not in pairs]
    bpairs, brows = dress(keys)
    st = check(ctx, n, n, pairs, rows, bpairs, brows)
    assert st[0] >= 5 + 4 and st[1] >= 5 + 20


LONG = 5000
RUN = [(3 << 40) + 3 * j for j in range(LONG)]


@pytest.mark.parametrize("case", ["three", "below", "above", "interleaved", "inline-gains-run", "inline-in-the-middle"])
def test_runs_longer_than_a_workgroup(ctx, case):
    """A pair of m with 5000 ids gains one id below all, one above all and one in the middle as one batch run, or one of them as an
    inline id, or a run of 5000 ids interleaved one by one with its own; a single inline pair gains a 5000-id run below, around
    or above it.  The ids kernel finds every element by co-rank, and stats[5] is the longest out row."""
    pairs, rows = multigraph(77, 300, 600)
    key = (150, 150)
    below, middle, above = RUN[0] - 5, RUN[LONG // 2] + 1, RUN[-1] + 7
    if case in ("three", "below", "above", "interleaved"):
        pairs[key], rows[key] = MULTI, RUN
        b = {"three": [below, middle, above], "below": [below], "above": [above], "interleaved": [x + 1 for x in RUN]}[case]
    else:
        pairs[key] = RUN[0] - 1 if case == "inline-gains-run" else middle
        rows.pop(key, None)
        b = RUN
    others, orows = batch_on(3, pairs, 300, 300, 40, 20)
    others.pop(key, None)
    orows.pop(key, None)
    bpairs = {**others, key: MULTI if len(b) > 1 else b[0]}
    brows = {**orows, **({key: b} if len(b) > 1 else {})}
    st, mo, mto = check(ctx, 300, 300, pairs, rows, bpairs, brows, keep_outputs=True)
    assert st[5] == {"three": LONG + 3, "below": LONG + 1, "above": LONG + 1, "interleaved": 2 * LONG, "inline-gains-run": LONG + 1,
                     "inline-in-the-middle": LONG + 1}[case]


def form_of(ctx, mat, nrows):
    """'hyper' or 'full', read off the device memory the snapshot holds, as tests/test_gpu_edges_remove.py reads it: the full
    form keeps nrows + 1 row pointers — 24 004 bytes at 6000 rows — and the hypersparse form of these tests (at most 60 stored
    rows, at most 1100 entries) holds 244 + 240 + 4400 + 8800 bytes, under 18 KiB with the pool's quarter of slack."""
    ctx.sync()
    before = ctx.device_bytes()[0]
    mat.free()
    ctx.sync()
    held = before - ctx.device_bytes()[0]
    assert held > 0
    return "full" if held >= 4 * (nrows + 1) else "hyper"


def prefer_hyper(nrows, populated):
    return "hyper" if nrows > 4096 and populated * 16 <= nrows else "full"    # fgpu_mat_from_coo's rule (mat.hip)


def sparse_rows(seed, n, rws, per_row, cols):
    """per_row entries on every row of rws, columns from `cols`, dressed as multigraph() dresses them"""
    rng = np.random.default_rng(seed)
    pairs, rows = {}, {}
    for a, r in enumerate(rws):
        for b, c in enumerate(rng.choice(cols, per_row, replace=False).tolist()):
            k = a * per_row + b
            if k % 4 == 0:
                pairs[(r, c)] = MULTI
                rows[(r, c)] = [(2 << 40) + 8 * k + j for j in range(2 + k % 3)]
            else:
                pairs[(r, c)] = (1 << 40) + k
    return pairs, rows


@pytest.mark.parametrize("case", ["hyper-stays", "hyper-to-full", "hyper-fwd-onto-full"])
def test_the_stored_forms(ctx, case):
    """6000 rows, columns from 30 values, so the transposed patterns are hypersparse throughout.  A hypersparse m of 40 populated
    rows and a batch on 10 new rows and on some of its own: 50 x 16 <= 6000, hypersparse.  The same m and a batch that populates
    400 rows: full.  A hypersparse fwd of 40 rows onto a full m of 400."""
    n = 6000
    rng = np.random.default_rng(40)
    cols = rng.choice(n, 30, replace=False)
    all_rows = np.sort(np.r_[rng.choice(np.arange(1, n - 1), 448, replace=False), [0, n - 1]]).tolist()
    few, many = all_rows[::9][:40], all_rows[1::9][:10]
    assert len(few) == 40 and few[0] == 0 and not set(few) & set(many)
    if case == "hyper-fwd-onto-full":
        pairs, rows = sparse_rows(41, n, sorted(set(all_rows[:400]) | {n - 1}), 1, cols)
        fresh, _ = sparse_rows(42, n, few, 10, cols)
        keys = sorted(fresh)
        m_hyper, b_hyper = False, True
    else:
        pairs, rows = sparse_rows(41, n, few[:-1] + [n - 1], 10, cols)          # 40 populated rows, the first and the last among them
        fresh, _ = sparse_rows(42, n, many if case == "hyper-stays" else all_rows[:400], 5 if case == "hyper-stays" else 1, cols)
        keys = sorted(fresh) + sorted(pairs)[::7]
        m_hyper, b_hyper = True, False
    bpairs, brows = dress(keys)
    st, mo, mto = check(ctx, n, n, pairs, rows, bpairs, brows, hyper=m_hyper, bhyper=b_hyper, keep_outputs=True)
    merged, _, _ = union_edges(pairs, rows, bpairs, brows)
    populated = len({r for r, _ in merged})
    want = {"hyper-stays": "hyper", "hyper-to-full": "full", "hyper-fwd-onto-full": "full"}[case]
    assert prefer_hyper(n, populated) == want and prefer_hyper(n, len({c for _, c in merged})) == "hyper"
    assert st[1] > 0 and st[0] > 0
    assert form_of(ctx, mo, n) == want
    assert form_of(ctx, mto, n) == "hyper"


def test_a_rectangular_matrix(ctx):
    """300 x 500: columns past the row dimension, and a transposed pattern of other dimensions than m."""
    pairs, rows = multigraph(500, 300, 3000, ncols=500)
    bpairs, brows = batch_on(4, pairs, 300, 500, 900, 450)
    assert max(c for _, c in bpairs) >= 300
    st = check(ctx, 300, 500, pairs, rows, bpairs, brows)
    assert st[0] == 450 and st[1] == 450 and st[2] > 0 and st[3] > 0


def seeded_edges(seed, n, count, first_id):
    rng = np.random.default_rng(seed)
    ids = first_id + rng.permutation(count)                               # the ids of a pair arrive in any order
    return np.stack([rng.integers(n, size=count), rng.integers(n, size=count), ids], axis=1).astype(U64)


def test_agreement_with_the_build(ctx):
    """Two multigraph edge lists A and B with disjoint ids over a 60 x 60 space: the union of their builds is the build of
    A ++ B in m_out, in mt_out and in every multi-edge row of a colliding pair."""
    n = 60
    A, B = seeded_edges(10, n, 4000, 1), seeded_edges(11, n, 3000, 10**6)
    fa, ba, ka, oa, ia = engine.edges_build(ctx, n, n, A[:, 0], A[:, 1], A[:, 2])
    fb, bb, kb, ob, ib = engine.edges_build(ctx, n, n, B[:, 0], B[:, 1], B[:, 2])
    AB = np.concatenate([A, B])
    fab, bab, kab, oab, iab = engine.edges_build(ctx, n, n, AB[:, 0], AB[:, 1], AB[:, 2])
    mo, mto, ok, oo, oi, st = engine.edges_union(ctx, fa, ba, ka, oa, ia, fb, bb, kb, ob, ib, stats=True)
    for got, want in ((mo, fab), (mto, bab)):
        for x, y in zip(got.export_csr(), want.export_csr()):
            assert (x is None and y is None) or np.array_equal(x, y)
    whole = {int(k): iab[int(oab[r]):int(oab[r + 1])].tolist() for r, k in enumerate(kab.tolist())}
    pa, pb = build_edges(A.tolist())[0], build_edges(B.tolist())[0]
    colliding = sorted((s << 32) | d for s, d in set(pa) & set(pb))
    assert len(colliding) > 500 and ok.tolist() == colliding and st[1] == len(colliding) and st[2] > 0 and st[3] > 0
    for r, k in enumerate(ok.tolist()):
        assert oi[int(oo[r]):int(oo[r + 1])].tolist() == whole[k]


def _raises_invalid(fn):
    with pytest.raises(_ffi.FgpuError) as e:
        fn()
    assert e.value.code == _ffi.FGPU_INVALID
    assert str(e.value).split(":", 1)[1].strip()   # fgpu_last_error is set


def test_rejections_leave_the_context_usable(ctx):
    pairs, rows = multigraph(303, 300, 2000)
    bpairs, brows = batch_on(5, pairs, 300, 300, 400, 200)
    m, mt = build(ctx, 300, 300, pairs)
    fwd, bwd = build(ctx, 300, 300, bpairs)
    rect, rect_t = build(ctx, 300, 64, multigraph(67, 300, 500, ncols=64)[0])
    boolean = ctx.mat_from_coo(300, 300, [1], [2])
    valued_t = ctx.mat_from_coo(300, 300, [1], [2], [3])
    a, b = flat(rows), flat(brows)
    single = next(k for k in sorted(pairs) if pairs[k] != MULTI)
    multi = next(k for k in sorted(rows) if len(rows[k]) >= 3)

    def call(mm=m, tt=mt, aa=a, ff=fwd, bb=bwd, rb=b):
        return engine.edges_union(ctx, mm, tt, *aa, ff, bb, *rb)

    def small(bp, br, ar=rows):
        f, t = build(ctx, 300, 300, bp)
        return lambda: engine.edges_union(ctx, m, mt, *flat(ar), f, t, *flat(br))

    def broken(rws, how):
        key, off, ids = (x.copy() for x in rws)
        if how == "descending":
            key = key[::-1].copy()
        elif how == "twice":
            key[1] = key[0]
        elif how == "short":
            ids = np.r_[ids[:1], ids[int(off[1]):]]
            off[1:] -= off[1] - U64(1)
        elif how == "swapped":
            ids[[0, 1]] = ids[[1, 0]]
        elif how == "equal":
            ids[1] = ids[0]
        elif how == "marker":
            ids[int(off[1]) - 1] = MULTI
        return key, off, ids

    cases = [
        lambda: call(mm=boolean),                                         # m not valued
        lambda: call(ff=boolean),                                         # fwd not valued
        lambda: call(tt=None),                                            # mt missing
        lambda: call(bb=None),                                            # bwd missing
        lambda: call(tt=valued_t),                                        # mt valued
        lambda: call(bb=valued_t),                                        # bwd valued
        lambda: call(tt=rect_t),                                          # mt of other dimensions
        lambda: call(bb=rect_t),                                          # bwd of other dimensions
        lambda: call(ff=rect, bb=rect_t),                                 # fwd of other dimensions than m
        lambda: call(aa=broken(a, "descending")),                         # keys descending
        lambda: call(rb=broken(b, "twice")),                              # a key twice
        lambda: call(aa=broken(a, "short")),                              # a run shorter than 2
        lambda: call(rb=broken(b, "short")),
        lambda: call(aa=broken(a, "swapped")),                            # ids descending in a run
        lambda: call(rb=broken(b, "equal")),                              # ... or repeated
        lambda: call(aa=broken(a, "marker")),                             # the marker as an id of a row
        lambda: call(rb=broken(b, "marker")),
        small({multi: 5}, {}, {k: v for k, v in rows.items() if k != multi}),        # MULTI_EDGE in m, no a row
        small({single: MULTI}, {}),                                                  # MULTI_EDGE in fwd, no b row
        small({single: pairs[single]}, {}),                                          # both sides: inline = inline
        small({single: MULTI}, {single: sorted([3, pairs[single]])}),                # ... the inline id in a b run
        small({multi: rows[multi][1]}, {}),                                          # ... an id of the a run = the inline id
        small({multi: MULTI}, {multi: [3, rows[multi][-1]]}),                        # ... run and run share an id
    ]
    ctx.sync()
    for bad in cases:
        before = ctx.device_bytes()[0]
        _raises_invalid(bad)
        ctx.sync()
        assert ctx.device_bytes()[0] == before, "a rejected call keeps device memory"
        check(ctx, 300, 300, pairs, rows, bpairs, brows)                  # the next call is exact
    # ignored: an a key that is not MULTI_EDGE in m, an a key on a pair the batch does not name or m does not hold, a b key that
    # is not MULTI_EDGE in fwd
    lone = next(k for k in sorted(bpairs) if bpairs[k] != MULTI)
    absent = next((299, c) for c in range(300) if (299, c) not in pairs and (299, c) not in bpairs)
    extra_a = {**rows, single: [1, 2], absent: [3, 4]}
    extra_b = {**brows, lone: [5, 6]}
    mo, mto, ok, oo, oi, st = engine.edges_union(ctx, m, mt, *flat(extra_a), fwd, bwd, *flat(extra_b), stats=True)
    merged, out, want_st = union_edges(pairs, rows, bpairs, brows)
    assert st == want_st and np.array_equal(oi, flat(out)[2])
    assert_matrix(mo, 300, 300, merged, True)


def test_a_call_keeps_no_device_memory(ctx):
    """As tests/test_gpu_edges_remove.py: warm, read in_use, call again, free what came back — in_use is where it was."""
    pairs, rows = multigraph(304, 5000, 20000)
    bpairs, brows = batch_on(7, pairs, 5000, 5000, 6000, 3000)
    m, mt = build(ctx, 5000, 5000, pairs)
    fwd, bwd = build(ctx, 5000, 5000, bpairs)
    a, b = flat(rows), flat(brows)

    def call():
        res = engine.edges_union(ctx, m, mt, *a, fwd, bwd, *b, stats=True)
        plain = (res[0].nvals, res[1].nvals, res[2].tolist(), res[3].tolist(), res[4].tolist(), res[5])
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


@pytest.mark.parametrize("form", ["full", "hyper"])
def test_union_then_remove_gives_back_the_inputs(ctx, form):
    """The shapes of test_a_call_keeps_no_device_memory: the batch joins, then every id of the batch leaves again through
    fgpu_edges_remove, with the union's out rows and the batch-only b rows as the multi-edge rows.  What is left is m and mt entry
    for entry: a promoted pair is demoted to the id it held, an extended pair keeps its own run, a pair only the batch named is
    emptied.  Once over matrices stored full and once with the base, and the union's output before it goes to the removal,
    stored hypersparse: both entry points search both forms."""
    n, hyper = 5000, form == "hyper"
    pairs, rows = multigraph(304, n, 20000)
    bpairs, brows = batch_on(7, pairs, n, n, 6000, 3000)
    m, mt = build(ctx, n, n, pairs, hyper)
    fwd, bwd = build(ctx, n, n, bpairs)
    mo, mto, ok, oo, oi = engine.edges_union(ctx, m, mt, *flat(rows), fwd, bwd, *flat(brows))
    if hyper:
        rp, ci, vals = mo.export_csr()
        r = np.repeat(np.arange(n), np.diff(rp).astype(np.int64))
        mo = build(ctx, n, n, dict(zip(zip(r.tolist(), ci.tolist()), vals.tolist())), hyper=True)[0]
    supplied = {k: v for k, v in brows.items() if k not in pairs}
    supplied.update({(k >> 32, k & 0xFFFFFFFF): oi[int(oo[j]):int(oo[j + 1])].tolist() for j, k in enumerate(ok.tolist())})
    t = np.array([(s, d, x) for (s, d), v in bpairs.items() for x in (brows[(s, d)] if v == MULTI else [v])], dtype=U64)
    sk, so, si = flat(supplied)
    m2, mt2, hit, taken, er, ec = engine.edges_remove(ctx, mo, mto, t[:, 0], t[:, 1], t[:, 2], sk, so, si)
    assert_matrix(m2, n, n, pairs, True)
    assert_matrix(mt2, n, n, transposed(pairs), False)
    assert len(hit) == len(t) and hit.all()
    assert list(zip(er.tolist(), ec.tolist())) == sorted(k for k in bpairs if k not in pairs)
    assert np.array_equal(taken, np.isin(si, t[:, 2]).astype(np.uint8))
