"""GPU: the stable sorts and builders of the matrix layer on wide id spaces, against the plain numpy references of
tests/wide_keys.py and tests/matrix_edges.py (tests/test_wide_keys_cpu.py and tests/test_matrix_edges_cpu.py hold the builders
to what they claim; tests/test_sort_plan_cpu.py walks the shape decisions themselves on the host).

1. The key-width ladder: every digit split and geometry the sorts of transpose.hip pick between 22 and 28 key bits — the
   staged form's (7,7,8) .. (9,9,9) and its four levels, the two-level form up to its last geometry and its refusal — through
   transpose, mat_from_coo and edges_build in every transpose_mode, a few thousand entries each.  Every cell states through the
   profiler scopes which form ran.  Nothing as long as a dimension is built on the host's side: dims, nvals, one full-range
   extract() (storage order: a wrong row pointer, a lost segment, an unstable level all show) and probes.
2. Column ids past 2^31 through the sort-and-unique classes (all six callers) and the entry-sized operations.
3. Row ids past 2^31 where memory follows the entries and the stored rows."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402
import wide_keys as wk  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
ALL = 2 ** 64 - 1
SORT_SCOPE = "segsort_unique (product rows)"


def profiled(ctx, fn):
    """fn() under the kernel profiler: (its result, {scope: ms})."""
    ctx.prof_enable(True)
    try:
        out = fn()
        scopes = {p["kernel"]: p["ms"] for p in ctx.prof_read()}
    finally:
        ctx.prof_enable(False)
    return out, scopes


def check_matrix(M, nrows, ncols, rows, cols, vals, what):
    """dims, nvals, the whole content in storage order, and a probe of every stored coordinate and its neighbours."""
    assert (M.nrows, M.ncols) == (nrows, ncols), what
    assert M.nvals == len(rows), what
    assert M.has_values == (vals is not None), what
    r, c, v = M.extract(0, ALL)
    np.testing.assert_array_equal(r, rows, err_msg=f"{what}: rows")
    np.testing.assert_array_equal(c, cols, err_msg=f"{what}: columns")
    if vals is not None:
        np.testing.assert_array_equal(v, vals, err_msg=f"{what}: values")
    else:
        assert v is None, what
    pr, pc, exp = wk.probe_coords(rows, cols)
    p, pv = M.probe(pr, pc, want_vals=True)
    np.testing.assert_array_equal(p, exp, err_msg=f"{what}: probe")
    want = np.zeros(len(pr), dtype=U64)
    if vals is not None:
        stored = dict(zip(zip(rows.tolist(), cols.tolist()), vals.tolist()))
        want = wk.u64([stored.get(k, 0) for k in zip(pr.tolist(), pc.tolist())])
    np.testing.assert_array_equal(pv, want, err_msg=f"{what}: probed values")


# =====================================================================================================================
# 1. the key-width ladder
# =====================================================================================================================
MODES = (0, 1, 2, 3)
OPS = ("transpose", "transpose-valued", "coo-tall", "coo-tall-valued", "coo-wide", "coo-wide-valued", "edges-rows", "edges-cols")
SQUARE_OPS = ("coo-square", "coo-square-valued")            # at the four-level width only: there is no cheaper shape for it
CELLS = [(n, m, op) for n in wk.LADDER for m in MODES for op in OPS + (SQUARE_OPS if n == wk.LADDER[-1] else ())]


def check_form(scopes, nkeys, mode, op, path=None):
    """Which sort ran, by the profiler scopes of the call (and edges_build's path counter)."""
    names = set(scopes)
    ks = {s for s in names if s.startswith("ks_")}
    kp = {s for s in names if s.startswith("kp_")}
    l3, l4 = "kp_scatter_kernel L3" in names, "kp_scatter_kernel L4" in names
    four = wk.staged_levels(nkeys) == 4
    assert four == (nkeys == (1 << 27) + 1)
    two_level = nkeys <= wk.TWO_LEVEL_MAX
    what = (nkeys, mode, op, sorted(names))
    if op.startswith("edges"):
        # the tuple sort picks its form as the builders do, whatever the mode says about rebuilding; where neither form
        # applies it sorts by 16-bit digits: two staged sorts of two levels each
        if mode in (0, 2):
            assert l3 and l4 == four and path == 1, what
        elif two_level:
            assert "ks_bucket_kernel" in names and not l3 and not l4 and path == 1, what
        else:
            assert path == 2 and "kp_scatter_kernel L2" in names and not l3 and not l4, what
        return
    if mode == 1:
        assert not ks and not kp, what
    elif mode == 3:
        assert ("ks_bucket_kernel" in names) == two_level and not kp, what
        assert two_level or not ks, what
    else:
        assert l3 and l4 == four and ("kp_count_kernel L4" in names) == four, what
        if mode == 2 or op.startswith(("transpose", "coo-square")):   # (mode 0 sorts the 300 keys of the narrow side in two levels)
            assert not ks, what


@pytest.mark.parametrize("nkeys,mode,op", CELLS, ids=[f"keys{n}-mode{m}-{op}" for n, m, op in CELLS])
def test_ladder_cell(ctx, nkeys, mode, op):
    """One operation at one key width in one transpose_mode; every matrix of the cell is freed before the next one."""
    mats, path = [], None
    with ctx.options(transpose_mode=mode):
        if op.startswith("transpose"):
            t = wk.transpose_case(nkeys)
            valued = op.endswith("valued")
            A = ctx.mat_from_csr(wk.NARROW, nkeys, t["rowptr"], t["colidx"], vals=t["vals"] if valued else None)
            At, scopes = profiled(ctx, A.transpose)
            mats = [A, At]
            check_matrix(At, nkeys, wk.NARROW, t["t_rows"], t["t_cols"], t["t_vals"] if valued else None, (nkeys, mode, op))
            check_matrix(A, wk.NARROW, nkeys, t["rows"], t["cols"], t["vals"] if valued else None, (nkeys, mode, op, "input"))
        elif op.startswith("coo"):
            c = wk.coo_case(nkeys, op.split("-")[1])
            valued = op.endswith("valued")
            M, scopes = profiled(ctx, lambda: ctx.mat_from_coo(c["nrows"], c["ncols"], c["rows"], c["cols"],
                                                               c["vals"] if valued else None))
            mats = [M]
            check_matrix(M, c["nrows"], c["ncols"], c["ref_rows"], c["ref_cols"], c["ref_vals"] if valued else None,
                         (nkeys, mode, op))
        else:
            e = wk.edges_case(nkeys, op.split("-")[1])
            (fwd, bwd, mkey, moff, mids, st), scopes = profiled(
                ctx, lambda: engine.edges_build(ctx, e["nrows"], e["ncols"], e["srcs"], e["dsts"], e["ids"], stats=True))
            mats, path = [fwd, bwd], st[7]
            check_matrix(fwd, e["nrows"], e["ncols"], e["fwd_rows"], e["fwd_cols"], e["fwd_vals"], (nkeys, mode, op, "fwd"))
            check_matrix(bwd, e["ncols"], e["nrows"], e["bwd_rows"], e["bwd_cols"], None, (nkeys, mode, op, "bwd"))
            np.testing.assert_array_equal(mkey, e["multi_key"])
            np.testing.assert_array_equal(moff, e["multi_off"])
            np.testing.assert_array_equal(mids, e["multi_ids"])
            assert st[0] == len(e["fwd_rows"]) and st[1] == len(e["multi_key"]) and st[2] == len(e["multi_ids"])
    in_use, pooled = ctx.device_bytes()
    forms = sorted(s for s in scopes if s.startswith(("ks_", "kp_")))
    print(f"\nWIDE cell keys={nkeys} mode={mode} op={op} path={path} in_use={in_use} pooled={pooled} forms={forms}")
    for m in mats:
        m.free()
    check_form(scopes, nkeys, mode, op, path)


def test_every_form_of_the_ladder_has_a_cell():
    """The table of DESIGN.md, from the cells' own parameters: each staged split and each two-level geometry is reached."""
    staged = {(wk.key_bits(n), wk.staged_levels(n)) for n, m, _ in CELLS if m in (0, 2)}
    assert staged == {(22, 3), (25, 3), (26, 3), (27, 3), (28, 4)}
    assert {n for n, m, _ in CELLS if m == 3 and n <= wk.TWO_LEVEL_MAX} == {1 << 22, (1 << 24) + 1, 1 << 26}
    assert {n for n, m, _ in CELLS if m == 3 and n > wk.TWO_LEVEL_MAX} == {(1 << 26) + 1, 1 << 27, (1 << 27) + 1}
    assert sum(1 for _, _, op in CELLS if op in SQUARE_OPS) == 2 * len(MODES)


# =====================================================================================================================
# 2. column ids past 2^31
# =====================================================================================================================
CALLERS = ("mxm", "from_coo", "merge", "merge-masks-dp", "merge-dm", "merge-dm-masks-dp")
LABELS = tuple(f"L{L}" for L in me.SORT_LENGTHS) + tuple(f"dup{d}" for d in me.DUP_COUNTS)
_sorted = {}


def dev(ctx, a: me.Csr):
    return ctx.mat_from_csr(a.nrows, a.ncols, a.rowptr, a.colidx)


def sorted_rows(ctx, caller, N):
    """One device call per (caller, key space) with every sort-class case in it: (rowptr, colidx, nvals, dims, the numpy
    reference, the profiler scopes).  These matrices have a few hundred rows: every array is entry-sized but the bitmaps of
    the big class."""
    if (caller, N) in _sorted:
        return _sorted[caller, N]
    sc = me.sort_cases(N)
    scopes = {}
    if caller == "mxm":
        F, B = dev(ctx, sc.F), dev(ctx, sc.B)
        got, scopes = profiled(ctx, lambda: F.mxm(B))
        ref = sc.C
        print(f"\nWIDE sort classes ncols={N}: {SORT_SCOPE} {scopes.get(SORT_SCOPE, -1.0):.3f} ms, device_bytes {ctx.device_bytes()}")
    elif caller == "from_coo":
        r, c = sc.coo()
        assert len(r) >= 4096
        with ctx.options(transpose_mode=1):                        # histogram, scatter, sort-and-unique per row
            got = ctx.mat_from_coo(sc.F.nrows, N, r, c)
        ref = sc.C
    else:
        m, dp, dm = sc.layers()
        masks = caller.endswith("masks-dp")
        if "-dm" not in caller:
            dm = None
        with ctx.options(merge_mode=1):                            # one wavefront per row, dirty rows sorted
            got = dev(ctx, m).merge(dev(ctx, dp), dev(ctx, dm) if dm is not None else None, dm_masks_dp=masks)
        ref = me.merge(m, dp, dm, masks)
    rp, ci, _ = got.export_csr()
    _sorted[caller, N] = (rp.copy(), ci.copy(), got.nvals, (got.nrows, got.ncols), ref, set(scopes))
    got.free()
    return _sorted[caller, N]


@pytest.mark.parametrize("N", me.WIDE_KEY_SPACES, ids=lambda n: f"ncols{n}")
@pytest.mark.parametrize("caller", CALLERS)
def test_wide_sort_classes_whole_result(ctx, caller, N):
    """All sort-class cases of a key space past 2^31 in ONE call, keys up to N - 1 = one below the padding value's
    neighbourhood, equal the numpy reference; the product ran its sort."""
    rp, ci, nvals, dims, ref, scopes = sorted_rows(ctx, caller, N)
    assert dims == (ref.nrows, ref.ncols) and nvals == ref.nnz
    np.testing.assert_array_equal(rp, ref.rowptr)
    np.testing.assert_array_equal(ci, ref.colidx)
    assert int(ci.max()) == N - 1
    if caller == "mxm":
        assert SORT_SCOPE in scopes, sorted(scopes)


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("N", me.WIDE_KEY_SPACES, ids=lambda n: f"ncols{n}")
@pytest.mark.parametrize("caller", CALLERS)
def test_wide_sort_classes_rows_of_one_length(ctx, caller, N, label):
    """The rows of one pre-unique length (its four overlap patterns, or one all-duplicate row), row by row."""
    rp, ci, _, _, ref, _ = sorted_rows(ctx, caller, N)
    sc = me.sort_cases(N)
    rows = [(i, name) for i, (name, _, _) in sc.claims.items() if name.split("-")[0] == label]
    assert len(rows) == (1 if label.startswith("dup") else len(me.SORT_PATTERNS))
    for i, name in rows:
        got = ci[int(rp[i]):int(rp[i + 1])]
        np.testing.assert_array_equal(got, ref.row(i), err_msg=f"{caller} ncols {N} {name} (row {i})")
        if caller in ("mxm", "from_coo"):
            assert len(got) == sc.claims[i][2], name


def wide_mat(ctx, N, rows, form, salt=None, ncols=None, nrows=wk.WIDE_ROWS):
    """{row: columns} on the device in the dense-row-pointer or the hypersparse form, valued when a salt is given."""
    r, c = wk.coords_of(rows)
    vals = wk.value_of(r, c, salt) if salt is not None else None
    if form == "hyper":
        rp, ci, hr = wk.hyper_arrays(rows)
        return ctx.mat_from_csr(nrows, ncols or N, rp, ci, vals=vals, hyper_rows=hr)
    rp, ci = wk.dense_arrays(nrows, rows)
    return ctx.mat_from_csr(nrows, ncols or N, rp, ci, vals=vals)


def content(mat):
    """(sorted coordinates, values or None) by export_csr: a few dozen rows."""
    rp, ci, v = mat.export_csr()
    rows = np.repeat(np.arange(mat.nrows, dtype=U64), np.diff(rp.astype(np.int64)))
    return list(zip(rows.tolist(), ci.tolist())), (v.tolist() if v is not None else None)


def values(coords, salt):
    return wk.value_of([k[0] for k in coords], [k[1] for k in coords], salt).tolist()


@pytest.mark.parametrize("valued", [False, True], ids=["pattern", "valued"])
@pytest.mark.parametrize("form", ["dense", "hyper"])
@pytest.mark.parametrize("N", me.WIDE_KEY_SPACES, ids=lambda n: f"ncols{n}")
def test_column_ids_past_2_31_through_the_entry_sized_operations(ctx, N, form, valued):
    """70 rows whose stored columns are 0, 2^31 - 1, 2^31, 2^31 + 1, N - 2, N - 1 and a run across 2^31: export, extract
    windows, probe (stored, neighbours, (r, N), (r, 2^32 + c)), resize across bit 31 both ways, merge with layers that
    straddle 2^31, intersect."""
    H = wk.HALF
    x, y, z = (wk.straddle_rows(N, s) for s in (0, 1, 2))
    sx, sy, sz = wk.as_set(x), wk.as_set(y), wk.as_set(z)
    salt = (lambda s: s) if valued else (lambda s: None)
    X, Y, Z = wide_mat(ctx, N, x, form, salt(0)), wide_mat(ctx, N, y, form, salt(1)), wide_mat(ctx, N, z, form)
    keys = sorted(sx)
    vd = dict(zip(keys, values(keys, 0)))
    assert (X.nrows, X.ncols, X.nvals, X.has_values) == (wk.WIDE_ROWS, N, len(keys), valued)
    assert content(X) == (keys, [vd[k] for k in keys] if valued else None)
    # extract windows
    for lo, hi in ((0, ALL), (0, 0), (1, 1), (63, 65), (66, wk.WIDE_ROWS - 1), (2, 4), (wk.WIDE_ROWS - 1, ALL), (wk.WIDE_ROWS, ALL), (5, 3)):
        sub = [k for k in keys if lo <= k[0] <= hi]
        r, c, v = X.extract(lo, hi)
        assert list(zip(r.tolist(), c.tolist())) == sub, (lo, hi)
        assert (v.tolist() if v is not None else None) == ([vd[k] for k in sub] if valued and sub else None), (lo, hi)
    # probe
    coords = []
    for r, c in keys:
        coords += [(r, c), (r, c + 1), (r, N), (r, (1 << 32) + c), (r + (1 << 32), c), (r, c ^ H)]
        if c:
            coords.append((r, c - 1))
    coords += [(0, ALL), (wk.WIDE_ROWS, 0), (wk.WIDE_ROWS - 1, N - 1), (wk.WIDE_ROWS - 1, 0xFFFFFFFF), (2, H)]
    p, pv = X.probe([k[0] for k in coords], [k[1] for k in coords], want_vals=True)
    assert p.tolist() == [int(k in sx) for k in coords]
    assert pv.tolist() == [vd[k] if valued and k in sx else 0 for k in coords]
    # resize: growing across bit 31 keeps everything, shrinking clips at bit 31
    low = {r: [c for c in cs if c < H - 3] for r, cs in x.items()}
    low = {r: cs for r, cs in low.items() if cs}
    G = wide_mat(ctx, N, low, form, salt(0), ncols=H - 3).resize(wk.WIDE_ROWS, N)
    gk = sorted(wk.as_set(low))
    assert (G.nrows, G.ncols) == (wk.WIDE_ROWS, N) and content(G) == (gk, [vd[k] for k in gk] if valued else None)
    for nc in (H, H + 1, H - 1, N - 1):
        S = X.resize(wk.WIDE_ROWS, nc)
        sub = [k for k in keys if k[1] < nc]
        assert 0 < len(sub) < len(keys) and (S.nrows, S.ncols) == (wk.WIDE_ROWS, nc)
        assert content(S) == (sub, [vd[k] for k in sub] if valued else None), nc
    S = X.resize(64, N)                                            # rows only: every column id survives
    sub = [k for k in keys if k[0] < 64]
    assert content(S) == (sub, [vd[k] for k in sub] if valued else None)
    # merge
    vy = dict(zip(sorted(sy), values(sorted(sy), 1)))
    for masks in (False, True):
        want = sorted(wk.merged(sx, sy, sz, masks))
        for mode in (0, 1, 2):
            with ctx.options(merge_mode=mode):
                got = X.merge(Y, Z, dm_masks_dp=masks)
            wv = None
            if valued:                                             # dp's value wins on a shared coordinate
                wv = [vy[k] if k in sy and not (masks and k in sz) else vd[k] for k in want]
            assert content(got) == (want, wv), (masks, mode)
            pat = X.merge_pattern(Y, Z, dm_masks_dp=masks)
            assert content(pat) == (want, None), (masks, mode)
    assert content(X.merge(None, Z))[0] == sorted(sx - sz) and content(X.merge(Y, None))[0] == sorted(sx | sy)
    # intersect: the pattern of both, the values of b
    both = sorted(sx & sy)
    got = X.intersect(Y)
    assert content(got) == (both, [vy[k] for k in both] if valued else None)
    assert X.intersect_nvals(Y) == len(both) == Y.intersect_nvals(X) and X.intersect_nvals(X) == len(keys)
    assert content(Z.intersect(X))[0] == sorted(sx & sz)


# =====================================================================================================================
# 3. row ids past 2^31
# =====================================================================================================================
def test_row_ids_past_2_31_where_memory_follows_the_entries(ctx):
    """2^32 - 2 rows, stored rows at 0, 2^31 - 1, 2^31, 2^31 + 1 and the last two: the hypersparse form from mat_from_csr
    and from the host path of mat_from_coo (fewer than 4096 tuples), read back by extract and probe.  export_csr, merge,
    resize, intersect and transpose allocate per row of the dimension (profiles/NOTES_wide_keys.md) and stay out."""
    N, H = wk.TALL_NROWS, wk.HALF
    rows = wk.tall_rows()
    keys = sorted(wk.as_set(rows))
    vd = dict(zip(keys, values(keys, 3)))
    rp, ci, hr = wk.hyper_arrays(rows)
    r, c = wk.coords_of(rows)
    rng = np.random.default_rng(32)
    pick = np.concatenate([np.arange(len(r)), rng.integers(0, len(r), 40)])   # every coordinate, 40 of them twice
    pick = rng.permutation(pick)
    tv = wk.u64(np.arange(len(pick))) + U64(1 << 50)
    last = wk.last_wins(r[pick], c[pick], tv)
    mats = {"csr": (ctx.mat_from_csr(N, 1000, rp, ci, hyper_rows=hr), None),
            "csr valued": (ctx.mat_from_csr(N, 1000, rp, ci, vals=wk.value_of(r, c, 3), hyper_rows=hr), vd),
            "coo": (ctx.mat_from_coo(N, 1000, r[pick], c[pick]), None),
            "coo valued": (ctx.mat_from_coo(N, 1000, r[pick], c[pick], tv), last)}
    coords = []
    for k in keys:
        coords += [k, (k[0] + 1, k[1]), (k[0] ^ H, k[1]), (k[0] + (1 << 32), k[1]), (k[0], k[1] + 1), (N, k[1])]
        if k[0]:
            coords.append((k[0] - 1, k[1]))
    coords += [(N - 1, 999), (0xFFFFFFFF, 0), (ALL, 0), (H, 1000)]
    windows = ((0, ALL), (0, 0), (1, H - 2), (H - 1, H - 1), (H - 1, H + 1), (H, H), (H + 2, N - 3), (N - 2, N - 1), (N - 1, ALL),
               (N, ALL), (H + 1, H))
    for name, (M, vals) in mats.items():
        assert (M.nrows, M.ncols, M.nvals, M.has_values) == (N, 1000, len(keys), vals is not None), name
        for lo, hi in windows:
            sub = [k for k in keys if lo <= k[0] <= hi]
            rr, cc, vv = M.extract(lo, hi)
            assert list(zip(rr.tolist(), cc.tolist())) == sub, (name, lo, hi)
            assert (vv.tolist() if vv is not None else None) == ([vals[k] for k in sub] if vals and sub else None), (name, lo, hi)
        p, pv = M.probe([k[0] for k in coords], [k[1] for k in coords], want_vals=True)
        assert p.tolist() == [int(k in vd) for k in coords], name
        assert pv.tolist() == [vals[k] if vals and k in vd else 0 for k in coords], name
