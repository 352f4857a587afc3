"""GPU parity at the edges of the matrix layer: the sort-and-unique size classes, the scan tiles, the builder thresholds, the
two storage forms and the thinly covered operations — every case against the plain numpy references of
tests/matrix_edges.py and, where the C oracle has the operation, against the oracle too (bit-exact).

The cases are built on the host by matrix_edges.py (tests/test_matrix_edges_cpu.py shows that they hold the lengths and
boundaries they name); all device calls go through the C ABI (include/fgpu.h)."""
import os
import struct
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
FGPU_INVALID, FGPU_DIM_MISMATCH = -3, -6
SORT_SCOPE = "segsort_unique (product rows)"


def dev(ctx, a: me.Csr, form="dense", vals=None):
    """`a` on the device in the dense-row-pointer or the hypersparse form (mat_from_csr)."""
    if form == "hyper":
        rp, hr = a.hyper()
        return ctx.mat_from_csr(a.nrows, a.ncols, rp, a.colidx, vals=vals, hyper_rows=hr)
    return ctx.mat_from_csr(a.nrows, a.ncols, a.rowptr, a.colidx, vals=vals)


def orc(a: me.Csr) -> oracle.CSR:
    return oracle.CSR(a.nrows, a.ncols, a.rowptr, a.colidx)


def assert_same(mat, ref, what=""):
    rp, ci, _ = mat.export_csr()
    assert (mat.nrows, mat.ncols) == (ref.nrows, ref.ncols), what
    assert mat.nvals == ref.nnz, what
    np.testing.assert_array_equal(rp, ref.rowptr, err_msg=str(what))
    np.testing.assert_array_equal(ci, ref.colidx, err_msg=str(what))


def triples(mat, lo=0, hi=2 ** 64 - 1):
    """extract() as (list of (row, col), list of values or None)."""
    r, c, v = mat.extract(lo, hi)
    return list(zip(r.tolist(), c.tolist())), (v.tolist() if v is not None else None)


def values_of(a: me.Csr, salt=0):
    return me.value_of(*a.pairs(), salt)


def value_dict(a: me.Csr, salt=0):
    r, c = a.pairs()
    return dict(zip(zip(r.tolist(), c.tolist()), me.value_of(r, c, salt).tolist()))


# =====================================================================================================================
# 1. sort-and-unique classes through three callers
# =====================================================================================================================
CALLERS = ("mxm", "from_coo", "merge", "merge-masks-dp", "merge-dm", "merge-dm-masks-dp")
LABELS = tuple(f"L{L}" for L in me.SORT_LENGTHS) + tuple(f"dup{d}" for d in me.DUP_COUNTS)
_sorted = {}


def sorted_rows(ctx, caller, N):
    """One device call per (caller, key space) with every sort-class case in it; returns (rowptr, colidx, nvals, the
    numpy reference, the oracle's result, the profiler scopes of the call)."""
    if (caller, N) in _sorted:
        return _sorted[caller, N]
    sc = me.sort_cases(N)
    scopes = set()
    if caller == "mxm":
        F, B = dev(ctx, sc.F), dev(ctx, sc.B)
        ctx.prof_enable(True)
        try:
            got = F.mxm(B)
            scopes = {p["kernel"] for p in ctx.prof_read()}
        finally:
            ctx.prof_enable(False)
        ref, orc_ref = sc.C, oracle.mxm(orc(sc.F), orc(sc.B))[0]
    elif caller == "from_coo":
        r, c = sc.coo()
        assert len(r) >= 4096                                      # the device build
        with ctx.options(transpose_mode=1):                        # histogram, scatter, sort-and-unique per row
            got = ctx.mat_from_coo(sc.F.nrows, N, r, c)
        ref, orc_ref = sc.C, oracle.build_csr(sc.F.nrows, N, r, c)
    else:
        m, dp, dm = sc.layers()
        masks = caller.endswith("masks-dp")
        if "-dm" not in caller:
            dm = None
        with ctx.options(merge_mode=1):                            # one wavefront per row, dirty rows sorted
            got = dev(ctx, m).merge(dev(ctx, dp), dev(ctx, dm) if dm is not None else None, dm_masks_dp=masks)
        ref = me.merge(m, dp, dm, masks)
        orc_ref = oracle.merge(orc(m), orc(dp), orc(dm) if dm is not None else None, masks)
    rp, ci, _ = got.export_csr()
    _sorted[caller, N] = (rp.copy(), ci.copy(), got.nvals, (got.nrows, got.ncols), ref, orc_ref, scopes)
    return _sorted[caller, N]


@pytest.mark.parametrize("N", me.KEY_SPACES, ids=lambda n: f"ncols{n}")
@pytest.mark.parametrize("caller", CALLERS)
def test_sort_classes_whole_result(ctx, caller, N):
    """All cases of one key space in ONE call — the three classes interleaved on the mid / big lists — equal the numpy
    reference and the oracle; the product ran its sort."""
    rp, ci, nvals, dims, ref, orc_ref, scopes = sorted_rows(ctx, caller, N)
    assert dims == (ref.nrows, ref.ncols) and nvals == ref.nnz == orc_ref.nnz
    np.testing.assert_array_equal(rp, ref.rowptr)
    np.testing.assert_array_equal(ci, ref.colidx)
    np.testing.assert_array_equal(rp, orc_ref.rowptr)
    np.testing.assert_array_equal(ci, orc_ref.colidx)
    if caller == "mxm":
        assert SORT_SCOPE in scopes, sorted(scopes)


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("N", me.KEY_SPACES, ids=lambda n: f"ncols{n}")
@pytest.mark.parametrize("caller", CALLERS)
def test_sort_classes_rows_of_one_length(ctx, caller, N, label):
    """The rows of one pre-unique length (its four overlap patterns, or one all-duplicate row), row by row."""
    rp, ci, _, _, ref, _, _ = sorted_rows(ctx, caller, N)
    sc = me.sort_cases(N)
    rows = [(i, name) for i, (name, _, _) in sc.claims.items() if name.split("-")[0] == label]
    assert len(rows) == (1 if label.startswith("dup") else len(me.SORT_PATTERNS))
    for i, name in rows:
        got = ci[int(rp[i]):int(rp[i + 1])]
        np.testing.assert_array_equal(got, ref.row(i), err_msg=f"{caller} ncols {N} {name} (row {i})")
        if caller in ("mxm", "from_coo"):
            assert len(got) == sc.claims[i][2], name


@pytest.mark.parametrize("k", [63, 64, 65, 66, 128, 129])
def test_mxm_sort_decision_with_a_partial_last_wavefront(ctx, k):
    """The product sorts when any F-row has two entries (gather_u64_kernel's wave maximum): here the only such row is the
    last one, in a wavefront of which all other lanes but the lane of entry k have left."""
    b = me.from_rows(4, 200, {0: [150, 160], 1: [10, 20, 155], 2: [5], 3: [7]})
    f = me.from_rows(k, 4, {**{i: [2 + i % 2] for i in range(k - 1)}, k - 1: [0, 1]})
    ref = me.mxm(f, b)
    assert ref.row(k - 1).tolist() == [10, 20, 150, 155, 160]
    assert_same(dev(ctx, f).mxm(dev(ctx, b)), ref, k)


# =====================================================================================================================
# 2. scan boundaries
# =====================================================================================================================
@pytest.mark.parametrize("nrows", me.SCAN_NROWS)
def test_scan_tile_boundaries(ctx, nrows):
    """nrows + 1 scanned counts on both sides of one and two 4096-item tiles, the populated rows at the tile edges."""
    a, p, d, b = me.scan_case(nrows)
    A, P, D, B = dev(ctx, a), dev(ctx, p), dev(ctx, d), dev(ctx, b)
    assert_same(A.intersect(P), me.intersect(a, p), "intersect")
    assert A.intersect_nvals(P) == me.intersect(a, p).nnz
    assert D.intersect_nvals(A) == me.intersect(d, a).nnz
    for mode in (0, 1, 2):
        with ctx.options(merge_mode=mode):
            for masks in (False, True):
                assert_same(A.merge(P, D, dm_masks_dp=masks), me.merge(a, p, d, masks), f"merge mode {mode} {masks}")
            assert_same(A.merge(P, None), me.merge(a, p, None), f"merge mode {mode} no dm")
    assert_same(A.mxm(B), me.mxm(a, b), "mxm")
    assert_same(A.col_slab(100, 200), me.clip(a, nrows, 200, col_lo=100), "col_slab")
    for lo, hi in ((0, nrows), (4090, min(nrows, 4100)), (nrows - 1, nrows), (1, nrows - 1)):
        assert_same(A.row_slab(lo, hi), me.clip(a, hi, me.SCAN_NCOLS, row_lo=lo), f"row_slab {lo} {hi}")
    for nr, nc in ((nrows - 2, 150), (nrows - 1, me.SCAN_NCOLS), (4095, 299)):
        if nr <= nrows:
            assert_same(A.resize(nr, nc), me.resize(a, nr, nc), f"resize {nr} {nc}")


def test_three_level_scan_on_a_hypersparse_matrix(ctx):
    """(1 << 24) + 4097 rows: the nrows + 1 counts of intersect need the three-level scan.  A dozen entries in rows 0, 4095,
    4096, 2^24 - 1, 2^24 and the last row, in hypersparse form.  Temporary device memory: the dense row pointers of `a`,
    the counts, their scan and the result's row pointers — four arrays of 64 MiB (plus the same 64 MiB on the host for
    extract()); nothing is exported as a CSR."""
    a, b = me.huge_case()
    n = me.HUGE_NROWS
    (arp, aci, ahr), (brp, bci, bhr) = me.hyper_arrays(a), me.hyper_arrays(b)
    A = ctx.mat_from_csr(n, me.HUGE_NCOLS, arp, aci, hyper_rows=ahr)
    B = ctx.mat_from_csr(n, me.HUGE_NCOLS, brp, bci, hyper_rows=bhr)
    sa = {(r, c) for r, cs in a.items() for c in cs}
    sb = {(r, c) for r, cs in b.items() for c in cs}
    inter = sorted(sa & sb)
    assert A.nvals == len(sa) and B.nvals == len(sb)
    assert A.intersect_nvals(B) == len(inter) == B.intersect_nvals(A)
    res = A.intersect(B)
    assert res.nvals == len(inter) and res.nrows == n
    assert triples(res)[0] == inter
    assert triples(res, 4096, 1 << 24)[0] == [x for x in inter if 4096 <= x[0] <= 1 << 24]
    coords = sorted(sa | sb) + [(n - 1, 1), (n, 0), (1 << 24, me.HUGE_NCOLS), (1, 0)]
    pr, pc = [x[0] for x in coords], [x[1] for x in coords]
    assert res.probe(pr, pc).tolist() == [int(x in sa and x in sb) for x in coords]
    assert A.probe(pr, pc).tolist() == [int(x in sa) for x in coords]


# =====================================================================================================================
# 3. thresholds
# =====================================================================================================================
@pytest.mark.parametrize("n", me.THRESHOLD_N)
@pytest.mark.parametrize("kind", ["bool", "uint64"])
def test_from_coo_at_the_host_device_switch(ctx, kind, n):
    """fgpu_mat_from_coo sorts fewer than 4096 tuples on the host and builds the rest on the device; on 50 x 50 almost
    every tuple is a duplicate, and a stored value is that of the LAST tuple of its coordinate on both sides."""
    r, c, v = me.heavy_dup_coo(n)
    M = ctx.mat_from_coo(50, 50, r, c, v if kind == "uint64" else None)
    assert_same(M, me.build(50, 50, r, c))
    assert_same(M, oracle.build_csr(50, 50, r, c))
    assert M.has_values == (kind == "uint64")
    pairs, vals = triples(M)
    want = me.last_wins(r, c, v)
    assert pairs == sorted(want)
    if kind == "uint64":
        assert vals == [want[k] for k in pairs]
        p, pv = M.probe(r[-200:], c[-200:], want_vals=True)
        assert p.all() and pv.tolist() == [want[k] for k in zip(r[-200:].tolist(), c[-200:].tolist())]
    else:
        assert vals is None


def build_and_transpose_twice(ctx, mode, nrows, ncols, r, c):
    ref = oracle.build_csr(nrows, ncols, r, c)
    mine = me.build(nrows, ncols, r, c)
    with ctx.options(transpose_mode=mode):
        A = ctx.mat_from_coo(nrows, ncols, r, c)
        assert_same(A, ref, "A")
        assert_same(A, mine, "A (numpy)")
        At = A.transpose()
        assert_same(At, oracle.transpose(ref), "At")
        assert_same(At, me.transpose(mine), "At (numpy)")
        assert_same(At.transpose(), ref, "Att")
    return A, At


@pytest.mark.parametrize("ncols", me.TRANSPOSE_NCOLS, ids=lambda n: f"ncols{n}")
@pytest.mark.parametrize("nnz", me.THRESHOLD_N, ids=lambda n: f"nnz{n}")
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=lambda m: f"mode{m}")
def test_transpose_thresholds(ctx, mode, nnz, ncols):
    """The counting transpose declines below 4096 entries, its staged levels start at a key space of 2^17, a key space of
    1 never takes them: every side of each, in every transpose_mode, with exactly nnz tuples and entries."""
    nrows, r, c = me.transpose_case(nnz, ncols)
    A, At = build_and_transpose_twice(ctx, mode, nrows, ncols, r, c)
    assert A.nvals == nnz == At.nvals


@pytest.mark.parametrize("shape", [(1, 70000), (70000, 1)], ids=["1x70000", "70000x1"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=lambda m: f"mode{m}")
def test_one_row_and_one_column_matrices(ctx, mode, shape):
    """A key space of ONE on either side of the builders and the transposes, with more than 4096 tuples and repeats."""
    r, c = me.thin_case(*shape)
    A, At = build_and_transpose_twice(ctx, mode, shape[0], shape[1], r, c)
    assert A.nvals == 5000 and (At.nrows, At.ncols) == (shape[1], shape[0])


def test_storage_form_flips_keep_the_content(ctx):
    """The host build goes hypersparse at nrows 4096 -> 4097 with 256 populated rows and back to dense row pointers at 256
    -> 257 populated rows: what can be observed (export, extract, probe) is the same on both sides."""
    r, c = me.hyper_flip_coo(256)
    r2, c2 = me.hyper_flip_coo(256, with_last_row=4096)
    v = me.value_of(r, c)
    want = me.last_wins(r, c, v)
    m4096 = ctx.mat_from_coo(4096, 4096, r, c, v)
    m4097 = ctx.mat_from_coo(4097, 4096, r, c, v)                 # 256 rows: hypersparse
    m257 = ctx.mat_from_coo(4097, 4096, r2, c2, me.value_of(r2, c2))   # 257 rows: dense row pointers
    assert_same(m4096, me.build(4096, 4096, r, c))
    assert_same(m4097, me.build(4097, 4096, r, c))
    assert_same(m257, me.build(4097, 4096, r2, c2))
    whole = triples(m4096)
    assert whole == (sorted(want), [want[k] for k in sorted(want)])
    assert triples(m4097) == whole and triples(m257, 0, 4095) == whole
    assert triples(m257, 4096, 4096)[0] == sorted(set(zip(r2.tolist(), c2.tolist())) - set(want))
    for lo, hi in ((0, 0), (4095, 4095), (1000, 3000), (4095, 2 ** 64 - 1)):
        sub = ([k for k in sorted(want) if lo <= k[0] <= hi], [want[k] for k in sorted(want) if lo <= k[0] <= hi])
        sub = sub if sub[0] else ([], None)
        assert triples(m4096, lo, hi) == sub and triples(m4097, lo, hi) == sub, (lo, hi)
    pr = np.concatenate([r, r, [4096, 4095]]).astype(U64)
    pc = np.concatenate([c, (c + U64(1)) % U64(4096), [0, 4095]]).astype(U64)
    exp = [(int(k in want), want.get(k, 0)) for k in zip(pr.tolist(), pc.tolist())]
    for m in (m4096, m4097):
        p, pv = m.probe(pr, pc, want_vals=True)
        assert list(zip(p.tolist(), pv.tolist())) == exp
    p, pv = m257.probe(pr[:-2], pc[:-2], want_vals=True)
    assert list(zip(p.tolist(), pv.tolist())) == exp[:-2]


# =====================================================================================================================
# 4. one content, two forms
# =====================================================================================================================
_forms = {}


def form_mats(ctx):
    """The three contents (x, y, z) on the device in both forms, with and without values."""
    if not _forms:
        for name, salt in (("x", 0), ("y", 1), ("z", 2)):
            a = me.form_content(salt)
            _forms[name] = a
            for form in me.FORMS:
                _forms[name, form, False] = dev(ctx, a, form)
                _forms[name, form, True] = dev(ctx, a, form, values_of(a, salt))
    return _forms


def empty_valued(ctx, form):
    z = np.zeros(0, dtype=U64)
    if form == "hyper":
        return ctx.mat_from_csr(me.FORM_N, 77, np.zeros(1, dtype=U64), z, vals=z, hyper_rows=z)
    return ctx.mat_from_csr(me.FORM_N, 77, np.zeros(me.FORM_N + 1, dtype=U64), z, vals=z)


def windows(a: me.Csr):
    """(name, min_row, max_row) over the populated rows of `a`."""
    live = np.nonzero(a.lengths())[0].tolist()
    gap = next((x + 1, y - 1) for x, y in zip(live, live[1:]) if y - x > 2)
    return [("min > max", 5, 3), ("min >= nrows", a.nrows, a.nrows + 5),
            ("the last row, max past the end", a.nrows - 1, 2 ** 64 - 1),
            ("max past the end", 4000, a.nrows + 100), ("only empty rows", gap[0], gap[1]),
            ("ends at the last populated row", live[-3], live[-1]), ("a single row", 4096, 4096),
            ("a single empty row", gap[0], gap[0]), ("row 0", 0, 0), ("around 4096", 4095, 4096)]


@pytest.mark.parametrize("form", me.FORMS)
def test_forms_unary_operations(ctx, form):
    f = form_mats(ctx)
    x = f["x"]
    vd = value_dict(x)
    keys = sorted(vd)
    for valued in (False, True):
        M = f["x", form, valued]
        assert M.has_values == valued
        assert_same(M, x, (form, valued))
        if valued:
            np.testing.assert_array_equal(M.export_csr()[2], values_of(x))
        assert triples(M) == (keys, [vd[k] for k in keys] if valued else None)
        for name, lo, hi in windows(x):
            sub = [k for k in keys if lo <= k[0] <= hi]
            want = (sub, [vd[k] for k in sub] if valued and sub else None)
            assert triples(M, lo, hi) == want, (form, valued, name)
        # probe: every stored coordinate, and its neighbours
        r, c = x.pairs()
        pr, pc = np.concatenate([r, r]), np.concatenate([c, (c + U64(1)) % U64(me.FORM_N)])
        p, pv = M.probe(pr, pc, want_vals=True)
        exp = [(int(k in vd), vd.get(k, 0) if valued else 0) for k in zip(pr.tolist(), pc.tolist())]
        assert list(zip(p.tolist(), pv.tolist())) == exp
        # transpose
        T = M.transpose()
        assert T.has_values == valued
        assert_same(T, me.transpose(x), ("transpose", form, valued))
        assert_same(T, oracle.transpose(orc(x)))
        tp, tv = triples(T)
        if valued:
            assert dict(zip(tp, tv)) == {(c_, r_): v for (r_, c_), v in vd.items()}
        assert_same(T.transpose(), x)
        # resize: grow keeps everything, shrink drops what falls outside
        G = M.resize(me.FORM_N + 4097, me.FORM_N + 1)
        assert G.has_values == valued and (G.nrows, G.ncols) == (me.FORM_N + 4097, me.FORM_N + 1)
        assert triples(G) == (keys, [vd[k] for k in keys] if valued else None)
        for nr, nc in ((4096, me.FORM_N), (4097, 2500), (1, 1)):
            S = M.resize(nr, nc)
            sub = [k for k in keys if k[0] < nr and k[1] < nc]
            assert_same(S, me.resize(x, nr, nc), ("shrink", form, valued, nr, nc))
            assert triples(S) == (sub, [vd[k] for k in sub] if valued and sub else None)
    # an empty valued matrix keeps its type through the transpose
    E = empty_valued(ctx, form)
    assert E.has_values and E.nvals == 0
    Et = E.transpose()
    assert Et.has_values and Et.nvals == 0 and (Et.nrows, Et.ncols) == (77, me.FORM_N)
    assert triples(Et) == ([], None) and triples(E) == ([], None)
    assert not ctx.mat_new(5, 5).has_values


@pytest.mark.parametrize("fa,fb", me.FORM_PAIRS, ids=[f"{a}-{b}" for a, b in me.FORM_PAIRS])
def test_forms_binary_operations(ctx, fa, fb):
    """merge (as m, as dp, as dm), intersect and mxm (as F, as B) with the left operand in form fa and the right one(s) in
    form fb: the same answer for every pair, the numpy reference's."""
    f = form_mats(ctx)
    x, y, z = f["x"], f["y"], f["z"]
    vx, vy = value_dict(x, 0), value_dict(y, 1)
    dead = z.to_set()
    for fd in me.FORMS:                                            # dm in both forms beside every (m, dp) pair
        for masks in (False, True):
            ref = me.merge(x, y, z, masks)
            for mode in (0, 1, 2):
                with ctx.options(merge_mode=mode):
                    got = f["x", fa, False].merge(f["y", fb, False], f["z", fd, False], dm_masks_dp=masks)
                assert_same(got, ref, ("merge", fa, fb, fd, masks, mode))
                assert not got.has_values
            assert_same(got, oracle.merge(orc(x), orc(y), orc(z), masks))
            # valued layers: dp's value wins on a shared coordinate
            want = {k: v for k, v in vx.items() if k not in dead}
            want.update({k: v for k, v in vy.items() if not (masks and k in dead)})
            got = f["x", fa, True].merge(f["y", fb, True], f["z", fd, False], dm_masks_dp=masks)
            assert got.has_values
            assert triples(got) == (sorted(want), [want[k] for k in sorted(want)]), (fa, fb, fd, masks)
            assert_same(got, ref)
            pat = f["x", fa, True].merge_pattern(f["y", fb, True], f["z", fd, True], dm_masks_dp=masks)
            assert not pat.has_values
            assert_same(pat, ref, ("merge_pattern", fa, fb, fd, masks))
    # z as the base, x as dp, y as dm: every content in every role
    assert_same(f["z", fa, False].merge(f["x", fb, False], f["y", fb, False]), me.merge(z, x, y))
    assert_same(f["x", fa, False].merge(None, f["y", fb, False]), me.merge(x, None, y))
    assert_same(f["x", fa, False].merge(f["y", fb, False], None), me.merge(x, y, None))
    # intersect: the pattern of both, the values of b
    for a_valued in (False, True):
        for b_valued in (False, True):
            got = f["x", fa, a_valued].intersect(f["y", fb, b_valued])
            ref = me.intersect(x, y)
            assert_same(got, ref, ("intersect", fa, fb, a_valued, b_valued))
            assert got.has_values == b_valued
            keys = sorted(x.to_set() & y.to_set())
            assert triples(got) == (keys, [vy[k] for k in keys] if b_valued else None)
            assert f["x", fa, a_valued].intersect_nvals(f["y", fb, b_valued]) == len(keys)
    # mxm: the structural product reads no value
    ref = me.mxm(x, y)
    assert_same(f["x", fa, False].mxm(f["y", fb, False]), ref, ("mxm", fa, fb))
    assert_same(f["x", fa, True].mxm(f["y", fb, True]), ref, ("mxm valued", fa, fb))
    assert_same(f["x", fa, False].mxm(f["y", fb, False]), oracle.mxm(orc(x), orc(y))[0])
    assert_same(f["y", fa, False].mxm(f["x", fb, False]), me.mxm(y, x), ("mxm y x", fa, fb))


def test_slabs_refuse_hypersparse_and_valued_inputs(ctx):
    f = form_mats(ctx)
    for key in (("x", "hyper", False), ("x", "dense", True), ("x", "hyper", True)):
        for slab in (f[key].col_slab, f[key].row_slab):
            with pytest.raises(engine.FgpuError) as e:
                slab(10, 4000)
            assert e.value.code == FGPU_INVALID
    x = f["x"]                                                     # the context still works
    assert_same(f["x", "dense", False].col_slab(10, 4000), me.clip(x, x.nrows, 4000, col_lo=10))
    assert_same(f["x", "dense", False].row_slab(10, 4097), me.clip(x, 4097, x.ncols, row_lo=10))


# =====================================================================================================================
# 5. thinly covered operations
# =====================================================================================================================
def rect_pair():
    """a, b of 300 x 7000: rows of 63 / 64 / 65 / 129 entries (and others) in a, b sharing about half of each row."""
    rng = np.random.default_rng(300)
    lens = (63, 64, 65, 129, 1, 128, 200, 2)
    a, b = {}, {}
    for n, r in enumerate([0, 1, 2, 3, 64, 65, 150, 151, 152, 298, 299]):
        x = np.sort(rng.choice(7000, lens[n % 8], replace=False))
        x[0], x[-1] = (0, 6999) if len(x) > 1 else (x[0], x[0])
        a[r] = x
        if n != 4:                                                 # (row 64 is in a only)
            b[r] = np.concatenate([x[::2], rng.integers(0, 7000, 40)])
    b[200] = [5, 6, 7]                                             # (a row in b only)
    return me.from_rows(300, 7000, a), me.from_rows(300, 7000, b)


@pytest.mark.parametrize("fa,fb", me.FORM_PAIRS, ids=[f"{a}-{b}" for a, b in me.FORM_PAIRS])
def test_intersect_rectangular_with_values_from_b(ctx, fa, fb):
    a, b = rect_pair()
    assert {63, 64, 65, 129} <= set(a.lengths().tolist())
    vb = value_dict(b, 5)
    keys = sorted(a.to_set() & b.to_set())
    assert 0 < len(keys) < a.nnz
    A, Av = dev(ctx, a, fa), dev(ctx, a, fa, values_of(a, 4))
    B, Bv = dev(ctx, b, fb), dev(ctx, b, fb, values_of(b, 5))
    E, Ev = ctx.mat_new(300, 7000), dev(ctx, me.from_rows(300, 7000, {}), fb, np.zeros(0, dtype=U64))
    got = A.intersect(Bv)                                          # values from b
    assert got.has_values and triples(got) == (keys, [vb[k] for k in keys]) and A.intersect_nvals(Bv) == len(keys)
    assert_same(got, me.intersect(a, b))
    got = Av.intersect(Bv)
    assert got.has_values and triples(got) == (keys, [vb[k] for k in keys])
    got = Av.intersect(B)                                          # a valued, b BOOL: no values
    assert not got.has_values and triples(got) == (keys, None) and Av.intersect_nvals(B) == len(keys)
    for x, y in ((A, E), (E, B), (Av, Ev), (E, E), (Ev, Bv)):      # either operand empty
        got = x.intersect(y)
        assert got.nvals == 0 and x.intersect_nvals(y) == 0 and triples(got) == ([], None)
        assert (got.nrows, got.ncols) == (300, 7000)
    got = Av.intersect(Av)                                         # identical operands
    va = value_dict(a, 4)
    assert triples(got) == (sorted(va), [va[k] for k in sorted(va)]) and Av.intersect_nvals(Av) == a.nnz
    r, c = a.pairs()
    shifted = me.build(300, 7000, (r + U64(1)) % U64(300), c)      # the same rows one row down ...
    d = me.from_keys(300, 7000, np.setdiff1d(shifted.keys(), a.keys()))
    D = dev(ctx, d, fb, values_of(d, 6))                           # ... without what they share: disjoint from a
    assert d.nnz and A.intersect_nvals(D) == 0 and A.intersect(D).nvals == 0
    assert_same(A.intersect(D), me.intersect(a, d))


def test_intersect_dimension_mismatch(ctx):
    a, _ = rect_pair()
    A = dev(ctx, a)
    for other in (ctx.mat_new(300, 7001), ctx.mat_new(301, 7000), ctx.mat_new(7000, 300)):
        with pytest.raises(engine.FgpuError) as e:
            A.intersect(other)
        assert e.value.code == FGPU_DIM_MISMATCH
        with pytest.raises(engine.FgpuError) as e:
            A.intersect_nvals(other)
        assert e.value.code == FGPU_DIM_MISMATCH
    assert A.intersect_nvals(A) == a.nnz                           # the context still works


@pytest.mark.parametrize("form", me.FORMS)
def test_probe_edges_with_values(ctx, form):
    f = form_mats(ctx)
    x = f["x"]
    vd = value_dict(x)
    M, P = f["x", form, True], f["x", form, False]
    n = me.FORM_N
    coords = []
    for r in np.nonzero(x.lengths())[0].tolist():
        first, last = int(x.row(r)[0]), int(x.row(r)[-1])
        coords += [(r, first), (r, last), (r, last + 1), (r + (1 << 32), first), (r + 1, first), (n + r, first)]
        if first:
            coords.append((r, first - 1))
    coords += [(n, 0), (0, n), (2 ** 64 - 1, 2 ** 64 - 1), (n - 1, n - 1 + (1 << 32)), (n - 1, n)]
    pr, pc = [k[0] for k in coords], [k[1] for k in coords]
    p, pv = M.probe(pr, pc, want_vals=True)
    assert list(zip(p.tolist(), pv.tolist())) == [(int(k in vd), vd.get(k, 0)) for k in coords]
    assert not any(k in vd for k in coords if k[0] >= n or k[1] >= n)
    p, pv = P.probe(pr, pc, want_vals=True)                        # BOOL: present, and 0 as the value
    assert p.tolist() == [int(k in vd) for k in coords] and not pv.any()
    assert P.probe(pr, pc).tolist() == p.tolist()
    p, pv = M.probe([], [], want_vals=True)                        # n = 0
    assert len(p) == 0 and len(pv) == 0
    for E in (ctx.mat_new(n, n), empty_valued(ctx, form)):         # an empty matrix
        p, pv = E.probe(pr, [min(c, 76) for c in pc], want_vals=True)
        assert not p.any() and not pv.any()


def f64_matrix(ctx, vals, form="dense"):
    """One row holding the given binary64 values."""
    bits = np.asarray(vals, dtype=np.float64).view(U64)
    n = len(bits)
    a = me.Csr(3, max(n, 1), [0, 0, n, n], np.arange(n))
    return dev(ctx, a, form, bits)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def min_bits(vals):
    """The minimum of the float64 view, as bits; -0.0 counts as +0.0."""
    m = float(np.min(np.asarray(vals, dtype=np.float64)))
    return 0 if m == 0.0 else f64_bits(m)


INF = float("inf")
MIN_CASES = {
    "negatives": [3.5, -2.25, -1e300, 7.0, -1e-300],
    "negative-zero-with-positive-zero": [5.0, -0.0, 0.0, 1e-300, INF],
    "negative-zero-alone": [2.0, -0.0, 3.0],
    "subnormal": [1.0, 5e-324, 2.0, 2.2250738585072014e-308],
    "negative-subnormal": [0.0, -5e-324, -0.0, 1.0],
    "inf-among-finite": [INF, 3.0, 9.0, INF],
    "only-inf": [INF, INF],
    "negative-inf": [1.0, -INF, -1.7976931348623157e308],
    "one-entry": [42.5],
    "one-negative-zero": [-0.0],
}


@pytest.mark.parametrize("case", sorted(MIN_CASES))
def test_min_val_special_values(ctx, case):
    vals = MIN_CASES[case]
    for form in me.FORMS:
        got = f64_matrix(ctx, vals, form).min_val()
        assert got is not None and f64_bits(got) == min_bits(vals), (case, form, got)
    if "negative-zero" in case:
        assert f64_bits(f64_matrix(ctx, vals).min_val()) == 0      # +0.0 exactly


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("n", [1025, 300001])
def test_min_val_over_blocks_and_grid_stride_trips(ctx, n, where):
    vals = np.random.default_rng(n).uniform(1.0, 2.0, n)
    vals[{"first": 0, "middle": n // 2 + 1, "last": n - 1}[where]] = 0.75
    got = f64_matrix(ctx, vals).min_val()
    assert f64_bits(got) == min_bits(vals) == f64_bits(0.75)
    vals[vals == 0.75] = -3.0
    assert f64_bits(f64_matrix(ctx, vals).min_val()) == f64_bits(-3.0)


def test_min_val_empty_bool_and_nan(ctx):
    assert ctx.mat_new(10, 10).min_val() is None
    assert empty_valued(ctx, "dense").min_val() is None and empty_valued(ctx, "hyper").min_val() is None
    assert ctx.mat_from_coo(10, 10, [3, 4], [5, 6]).min_val() == 1.0   # BOOL
    # the documented order: a positive NaN sorts above +inf and never wins
    nan = float(np.array([0x7FF8000000000000], dtype=U64).view(np.float64)[0])
    assert f64_bits(f64_matrix(ctx, [nan, INF, 5.0]).min_val()) == f64_bits(5.0)
    assert f64_bits(f64_matrix(ctx, [nan, INF]).min_val()) == f64_bits(INF)


@pytest.mark.parametrize("form", me.FORMS + ("empty",))
def test_row_degrees(ctx, form):
    import torch
    nrows = 4097
    if form == "empty":
        M = ctx.mat_new(nrows, 300)
    else:
        M = dev(ctx, me.scan_case(nrows)[0], form)
    # (-1 everywhere, by a copy from the host: no torch kernel has to be loaded for this test)
    deg = torch.from_numpy(np.full(nrows, -1, dtype=np.int32)).to("cuda:0")
    M.row_degrees(deg.data_ptr())
    torch.cuda.synchronize()
    want = np.diff(M.export_csr()[0].astype(np.int64))
    np.testing.assert_array_equal(deg.cpu().numpy(), want)
    assert int(want.sum()) == M.nvals and (form == "empty") == (M.nvals == 0)
    if form != "empty":
        assert want[0] and want[4095] and want[4096]
