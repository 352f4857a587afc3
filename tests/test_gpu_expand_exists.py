"""GPU: fgpu_expand_exists — bit i = row i of fgpu_expand over the same arguments is not empty — against the numpy statement of
that contract (tests/exists_check.py) AND against engine.expand's row degrees on the same inputs, in both forms of the last step
(sorted-CSR frontier / bit state), with the figures the call reports: rows matched, undecided rows sent through the exact pass
(equal to the decision rule's count, exists_check.decide), entries read, the form that ran.

The row-level mask of the last hop is the case a per-edge kernel gets wrong: test_mask_quirk fails on one.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import _ffi, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_graph as cg  # noqa: E402
import exists_check as ec  # noqa: E402
from test_gpu_chain_forms import ROWS, check_scopes, graphs, run  # noqa: E402,F401  (graphs: the cells' module fixture)
from test_gpu_expand_ownership import _Graph as OwnershipGraph, held_and_steady  # noqa: E402

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64
SKIP = cg.SKIP

CSR_K, PQ_K, BITS_K, LONG_K, DCOLS_K = ("exists_csr_kernel", "exists_pq_kernel", "exists_bits_kernel", "exists_long_rows_kernel",
                                        "exists_dm_cols_kernel")
PROBE = "bp_probe_rows_kernel"


def upload(ctx, c, hyper=False):
    """A host CSR on the device (None stays None); hyper: stored as its non-empty rows."""
    if c is None:
        return None
    if not hyper:
        return ctx.mat_from_coo(c.nrows, c.ncols, *c.pairs())
    deg = np.diff(c.rowptr.astype(I64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(c.nrows, c.ncols, short, c.colidx, hyper_rows=rows)


class Layers:
    """Host layers [(m, dp, dm)] and their device copies, freed together."""

    def __init__(self, ctx, host, hyper=False):
        self.host = host
        seen = {}
        for x in (x for layer in host for x in layer if x is not None):
            if id(x) not in seen:
                seen[id(x)] = upload(ctx, x, hyper)
        self._mats = list(seen.values())
        col = lambda j: [seen[id(layer[j])] if layer[j] is not None else None for layer in host]
        self.m, self.dp, self.dm = col(0), col(1), col(2)
        if all(x is None for x in self.dp):
            self.dp = None
        if all(x is None for x in self.dm):
            self.dm = None

    def free(self):
        for m in self._mats:
            m.free()


def bitmap(ncols, ids):
    return None if ids is None else oracle.bits_from_ids(ncols, np.asarray(ids, dtype=U64))


def agree(ctx, src, L, label=None, opts=None, expand_opts=None):
    """One call under `opts`, held to the contract, to engine.expand's row degrees and to the decision rule's figures.
    Returns (match, stats, launches)."""
    opts = opts or dict(expand_mode=0)
    n0, ncols = L.host[0][0].nrows, L.host[-1][0].ncols
    bits = bitmap(ncols, label)
    (got, flops, stats), launches = run(ctx, opts, lambda: engine.expand_exists(ctx, src, L.m, L.dp, L.dm, bits))
    want = ec.expected(src, L.host, n0, label)
    with cg.forced(ctx, **(expand_opts or opts)):
        rp, _, _ = engine.expand(ctx, src, L.m, L.dp, L.dm, bits)
    deg = np.diff(np.asarray(rp).astype(I64)) > 0
    print("stats", stats, "rows", len(src), "want", int(want.sum()))
    assert np.array_equal(want, deg)                    # (the two references agree with each other)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    sure, undecided = ec.decide(src, L.host, n0, label)
    assert stats[0] == int(want.sum()) and stats[1] == int(undecided.sum())
    assert flops == cg.reference(src, L.host[:-1], n0)[1]           # the hops that ran: every hop but the last
    return got, stats, launches


def form_scopes(stats, launches, form, dirty, walks):
    """stats[3] and the profiler scopes of the form that answered (`walks`: a label or D makes the rows be walked)."""
    assert stats[3] == (1 if form == "bits" else 0)
    must = {CSR_K: 1} if form == "csr" else {PQ_K: 1, BITS_K: 1}
    if form == "bits" and walks:
        must[LONG_K] = 1
    if dirty:
        must[DCOLS_K] = 1
    must_not = ([PQ_K, BITS_K, LONG_K] if form == "csr" else [CSR_K]) + [PROBE] + ([] if dirty else [DCOLS_K])
    for k, c in must.items():
        assert launches.get(k, 0) == c, (k, c, launches)
    for k in must_not:
        assert k not in launches, (k, launches)


# ---- the mask quirk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["csr", "bits"])
@pytest.mark.parametrize("name", list(ec.mask_cases()))
def test_mask_quirk(ctx, name, mode):
    src, layers, label, want, undecided = ec.mask_cases()[name]
    L = Layers(ctx, layers)
    try:
        got, stats, launches = agree(ctx, src, L, label, dict(expand_mode=mode))
    finally:
        L.free()
    assert np.array_equal(got, want)
    assert stats[1] == int(undecided.sum())
    if name == "masked":
        assert not got[0] and stats[1] >= 1               # a per-edge rule answers True through (u1, v)
    if name in ("plus (u1, v2)", "plus dp (u2, v3)"):
        assert got[0] and stats[1] == 0
    form = "bits" if mode == 2 and len(layers) > 1 else "csr"
    dirty = layers[-1][2] is not None
    form_scopes(stats, launches, form, dirty, dirty or label is not None)


# ---- the forms, on the cells of the chain's form decisions ------------------------------------------------------------------------
# cell (its chain is the exists call's nhops - 1 hops), the form the last step must run in
FORM_CELLS = {
    "1 mode 1": "csr",
    "2 dirty, push at 1 under mode 1": "csr",
    "7 probe, push at 1": "bits",
    "7 probe, compacted, scatter at 1": "bits",
    "7 probe, small, compacted, push at 1": "bits",
}


@pytest.mark.parametrize("label", [False, True], ids=["", "label"])
@pytest.mark.parametrize("cell", list(FORM_CELLS))
def test_forms(ctx, graphs, cell, label):
    form = FORM_CELLS[cell]
    if cell.endswith("under mode 1"):
        g, _, _ = graphs("2 dirty, push at 1")
        opts, row = dict(expand_mode=1, expand_bits_ratio=33), None
    else:
        g, _, opts = graphs(cell)
        row = ROWS[cell] if cell.startswith("7 probe") else None
    m, dp, dm = g.device_layers(ctx, 3)
    lab = cg.label_ids(g.n) if label else None
    want = ec.rows_nonempty(g.ref(3, label=label)[0])
    sure, undecided = ec.decide(g.src, g.layers(3), g.n, lab)
    (got, flops, stats), launches = run(ctx, opts, lambda: engine.expand_exists(ctx, g.src, m, dp, dm, g.label() if label else None))
    print(cell, g.figures(), stats)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    assert want.any() and (~want).any()
    assert flops == g.ref(2)[1]
    assert stats[0] == int(want.sum()) and stats[1] == int(undecided.sum())
    form_scopes(stats, launches, form, g.dirty, g.dirty or label)
    if row is not None and stats[1] == 0:
        # the chain before the last step is the cell's own: its scopes with the probe's last step replaced by this one
        must, must_not = dict(row[0]), list(row[1])
        must.pop(PROBE)
        check_scopes(launches, must, must_not)
    if form == "csr":
        assert not any(s.startswith("bp_") for s in launches), launches


# ---- row counts, in both forms ---------------------------------------------------------------------------------------------------
T, BASE = 200, 64 + 4 * 200          # thin chains t -> a -> b -> c of T vertices each behind 64 vertices without out-edges


class RandGraph:
    """One matrix for every hop.  Vertices < 64: no out-edge.  Thin chains t_i -> a_i -> b_i -> c_i: i % 4 == 0 has (b_i, c_i)
    tombstoned (no match), == 1 has c_i tombstoned from a vertex x_i the row never reaches (a match only the row-level rule
    gives: the exact pass), == 2 has a dp entry out of b_i as well, == 3 is plain.  From BASE on: v % 5 random out-edges, a fifth
    of them tombstoned, and 1 % as many dp entries."""

    def __init__(self, ctx, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        i = np.arange(T, dtype=I64)
        t, a, b, c = 64 + i, 64 + T + i, 64 + 2 * T + i, 64 + 3 * T + i
        v = np.arange(BASE, n, dtype=I64)
        rr = np.repeat(v, v % 5)
        rc = rng.integers(BASE, n, len(rr))
        x = BASE + 5 * i                                        # (x % 5 == 4: they have out-edges of their own)
        q1 = i % 4 == 1
        rows = np.concatenate([t, a, b, rr, x[q1]])
        cols = np.concatenate([a, b, c, rc, c[q1]])
        pick = rng.random(len(rr)) < 0.2
        q0, q2 = i % 4 == 0, i % 4 == 2
        dmr = np.concatenate([rr[pick], b[q0], x[q1]])
        dmc = np.concatenate([rc[pick], c[q0], c[q1]])
        ndp = max(len(rr) // 100, 1)
        dpr = np.concatenate([rng.integers(BASE, n, ndp), b[q2]])
        dpc = np.concatenate([rng.integers(0, n, ndp), c[q2] - 1])
        csr = lambda r, c_: oracle.build_csr(n, n, r.astype(U64), c_.astype(U64))
        self.a = csr(rows, cols)
        new = ~self.a.has_edges(dpr.astype(U64), dpc.astype(U64))          # dp adds entries, dm names entries m has
        assert self.a.has_edges(dmr.astype(U64), dmc.astype(U64)).all() and (x % 5 == 4).all()
        self.dp, self.dm = csr(dpr[new], dpc[new]), csr(dmr, dmc)
        self.t, self.av = t, a
        self.rng = rng
        self.dirty = Layers(ctx, [(self.a, self.dp, self.dm)])

    @staticmethod
    def _same(L, hops):
        o = object.__new__(Layers)
        o.host = L.host * hops
        o.m, o.dp, o.dm = L.m * hops, L.dp * hops, L.dm * hops
        o._mats = []
        return o

    def layers(self, hops):
        return self._same(self.dirty, hops)

    def sources(self, k, hops):
        """Skipped rows, sources without out-edges, thin chains (the vertex `hops` steps before c), one vertex many times over,
        the rest random."""
        i = np.arange(k, dtype=I64)
        kind = (i + 4) % 7
        thin = {3: self.t, 2: self.av}[hops]
        src = BASE + (i * 7919) % (self.n - BASE)
        src = np.where(kind == 1, i % 64, src)
        src = np.where(kind == 2, thin[(i // 7) % T], src)
        src = np.where(kind == 3, BASE + 9, src).astype(U64)
        src[kind == 0] = SKIP
        return src

    def free(self):
        self.dirty.free()


ROW_COUNTS = [1, 63, 64, 65, 1024, 1025, 4160]


@pytest.fixture(scope="module")
def dense_graph(ctx):
    g = RandGraph(ctx, 5003, 0xE715)
    yield g
    g.free()


@pytest.fixture(scope="module")
def sparse_graph(ctx):
    g = RandGraph(ctx, (1 << 19) + 1, 0xE716)
    yield g
    g.free()


@pytest.mark.parametrize("k", ROW_COUNTS)
def test_row_counts_bit_form(ctx, dense_graph, k):
    """Three hops under the default options: from 1025 rows on the two-hop chain over 5003 vertices ends in bits by itself (4160
    rows: 65 words a vertex, a stride of 128); the smaller batches are held to the bit form by expand_mode = 2."""
    g = dense_graph
    src = g.sources(k, 3)
    opts = dict(expand_mode=0) if k >= 1025 else dict(expand_mode=2)
    got, stats, launches = agree(ctx, src, g.layers(3), None, opts)
    form_scopes(stats, launches, "bits", True, True)
    if k >= 63:
        assert stats[1] >= 1 and got.any() and (~got).any()


@pytest.mark.parametrize("k", ROW_COUNTS)
def test_row_counts_csr_form(ctx, sparse_graph, k):
    """Three hops under the default options over 2^19 + 1 vertices: T * 28 stays below nnz, the chain never leaves the CSR form."""
    g = sparse_graph
    src = g.sources(k, 3)
    got, stats, launches = agree(ctx, src, g.layers(3), None, dict(expand_mode=0))
    form_scopes(stats, launches, "csr", True, True)
    if k >= 63:
        assert stats[1] >= 1 and got.any() and (~got).any()


@pytest.mark.parametrize("mode", [1, 2], ids=["csr", "bits"])
@pytest.mark.parametrize("k", [65, 1025])
def test_row_counts_two_hops_with_label(ctx, dense_graph, k, mode):
    g = dense_graph
    src = g.sources(k, 2)
    label = np.flatnonzero(np.arange(g.n) % 3 != 0).astype(U64)
    got, stats, launches = agree(ctx, src, g.layers(2), label, dict(expand_mode=mode))
    form_scopes(stats, launches, "bits" if mode == 2 else "csr", True, True)
    assert got.any() and (~got).any()


# ---- row lengths of the last matrix ----------------------------------------------------------------------------------------------
HN, HCOLS, HUB_LEN = 4097, 70071, 70000          # 4097 x 70071 last matrix: neither is a multiple of 64
HUB_FIRST, HUB_LAST = HCOLS - HUB_LEN, HCOLS - 1
# vertex: the columns of its row (lengths 0, 1, 63, 64, 65 and the hub)
LEN_ROWS = {
    3000: [],
    3001: [63],
    3002: list(range(1, 64)),
    3003: list(range(0, 64)),
    3004: list(range(0, 65)),
    3005: list(range(HUB_FIRST, HCOLS)),
}
LABELS = {
    "none": None,
    "bits 63, 64": [63, 64],              # the short rows pass (63 is the last entry of three of them), the hub does not
    "bit 64": [64],                       # only the 65-entry row, by its last entry
    "hub first": [HUB_FIRST],
    "hub last": [HUB_LAST],               # bit ncols - 1
    "nothing the rows hold": [65, 66],
}


@pytest.fixture(scope="module")
def length_layers(ctx):
    verts = np.array(sorted(LEN_ROWS), dtype=I64)
    r = np.concatenate([np.full(len(c), u, dtype=I64) for u, c in LEN_ROWS.items()]).astype(U64)
    c = np.concatenate([np.array(c, dtype=I64) for c in LEN_ROWS.values()]).astype(U64)
    last = oracle.build_csr(HN, HCOLS, r, c)
    dm = oracle.build_csr(HN, HCOLS, np.array([3001], dtype=U64), np.array([63], dtype=U64))     # the one entry of the 1-row
    # the first hop: source 10 + j -> vertex j of the table, one frontier vertex a row; and a few unrelated edges
    s = 10 + np.arange(len(verts), dtype=I64)
    hop0 = oracle.build_csr(HN, HN, np.concatenate([s, np.arange(2000, 2400)]).astype(U64),
                            np.concatenate([verts, np.arange(100, 500)]).astype(U64))
    made = {
        ("one", False): Layers(ctx, [(last, None, None)]),
        ("one", True): Layers(ctx, [(last, None, dm)]),
        ("two", False): Layers(ctx, [(hop0, None, None), (last, None, None)]),
        ("two", True): Layers(ctx, [(hop0, None, None), (last, None, dm)]),
    }
    yield made, verts, s
    for L in made.values():
        L.free()


# the bit form over the rectangular last matrix runs without an exact pass: clean, or with the labels under which the one
# tombstoned column (63) does not pass, so that D and the long rows meet there all the same
LENGTH_CASES = [(shape, label, dirty) for shape in ("one hop", "two hops, csr", "two hops, bits") for label in LABELS
                for dirty in (False, True)
                if not (shape.endswith("bits") and dirty and label in ("none", "bits 63, 64"))]


@pytest.mark.parametrize("shape,label,dirty", LENGTH_CASES)
def test_row_lengths(ctx, length_layers, shape, label, dirty):
    made, verts, s = length_layers
    one = shape == "one hop"
    L = made[("one" if one else "two", dirty)]
    src = np.concatenate([(verts if one else s).astype(U64), np.array([SKIP], dtype=U64)])
    mode = 2 if shape.endswith("bits") else 1
    # (engine.expand, the second reference, runs its sorted-CSR products: the rectangular last hop is not what is under test)
    got, stats, launches = agree(ctx, src, L, LABELS[label], dict(expand_mode=mode), expand_opts=dict(expand_mode=1))
    form_scopes(stats, launches, "bits" if mode == 2 and not one else "csr", dirty, dirty or LABELS[label] is not None)
    hub = int(np.flatnonzero(verts == 3005)[0])
    short = sum(len(c) for u, c in LEN_ROWS.items() if u != 3005)
    if label == "none" and not dirty:
        assert stats[2] == 0                              # row lengths alone: no entry is read
        assert got[hub] and not got[0]
    if label == "hub first":
        assert got[hub] and stats[2] <= 64 + short         # the wavefront stops at its first stride
    if label == "hub last":
        assert got[hub] and stats[2] >= HUB_LEN
    if label in ("bits 63, 64", "bit 64", "nothing the rows hold"):
        assert not got[hub] and stats[2] >= HUB_LEN
    if dirty and label == "none":
        assert not got[1] and stats[1] == 1               # the 1-entry row: its entry is tombstoned, only the exact pass says so
    if dirty and label == "bits 63, 64":
        assert not got[1] and got[2] and got[3] and stats[1] == 3    # ... and that the rows ending in 63 keep it


# ---- one hop does no pass over the vertices ----------------------------------------------------------------------------------------
def test_one_hop_reads_only_the_source_rows(ctx):
    n = 1 << 20
    rng = np.random.default_rng(0xE717)
    rows = np.repeat(rng.choice(n, 300, replace=False), 40).astype(U64)
    cols = rng.integers(0, n, len(rows)).astype(U64)
    m = oracle.build_csr(n, n, rows, cols)
    mr, mc = m.pairs()
    pick = rng.random(len(mr)) < 0.3
    dm = oracle.build_csr(n, n, mr[pick], mc[pick])
    dp = oracle.build_csr(n, n, rows[::9], rng.integers(0, n, len(rows[::9])).astype(U64))
    has = np.unique(rows)
    src = np.concatenate([has[:5], np.array([SKIP, 12345 if 12345 not in has else 12346], dtype=U64), has[5:6]]).astype(U64)
    assert len(src) == 8
    label = np.flatnonzero(oracle.mix64(np.arange(n, dtype=U64)) % U64(8) == 0).astype(U64)    # an eighth passes: rows are walked far
    for layer in ([(m, None, None)], [(m, dp, dm)]):
        L = Layers(ctx, layer, hyper=True)
        try:
            for lab in (None, label):
                got, stats, launches = agree(ctx, src, L, lab)
                dirty = layer[0][2] is not None
                form_scopes(stats, launches, "csr", dirty, dirty or lab is not None)
                bound = ec.row_lengths(src, layer[0][:2], n)       # the m and dp rows; the dm rows are not walked
                assert stats[2] <= bound, (stats, bound)
                if lab is None and not dirty:
                    assert stats[2] == 0
                assert not [s for s in launches if s.startswith("bp_")]
        finally:
            L.free()


# ---- errors, the empty call, ownership ----------------------------------------------------------------------------------------------
def test_errors_and_the_empty_call(ctx, dense_graph):
    g = dense_graph
    L = g.layers(2)
    src = g.sources(65, 2)
    with pytest.raises(_ffi.FgpuError) as e:
        engine.expand_exists(ctx, src, [])
    assert e.value.code == _ffi.FGPU_INVALID
    other = ctx.mat_new(g.n + 1, g.n + 1)
    try:
        with pytest.raises(_ffi.FgpuError) as e:
            engine.expand_exists(ctx, src, L.m, [L.dp[0], other], L.dm)
        assert e.value.code == _ffi.FGPU_DIM_MISMATCH
        with pytest.raises(_ffi.FgpuError) as e:
            engine.expand_exists(ctx, src, [L.m[0], other])
        assert e.value.code == _ffi.FGPU_DIM_MISMATCH
    finally:
        other.free()
    am = engine._hop_arrays(L.m)
    s = np.ascontiguousarray(src)
    code = ctx.lib.fgpu_expand_exists(ctx._h, s.ctypes.data_as(_ffi.u64p), len(s), am, None, None, 2, None, None, None, None)
    assert code == _ffi.FGPU_NULL_POINTER
    with pytest.raises(_ffi.FgpuError) as e:
        engine.expand_exists(ctx, np.array([g.n], dtype=U64), L.m)
    assert e.value.code == _ffi.FGPU_OUT_OF_BOUNDS
    got, flops, stats = engine.expand_exists(ctx, np.zeros(0, dtype=U64), L.m, L.dp, L.dm)
    assert len(got) == 0 and flops == 0 and stats == [0, 0, 0, 0]
    # nsrc == 0 leaves the caller's words alone
    w = np.full(1, 7, dtype=U64)
    assert ctx.lib.fgpu_expand_exists(ctx._h, None, 0, am, None, None, 2, None, w.ctypes.data_as(_ffi.u64p), None, None) == 0
    assert int(w[0]) == 7
    # every row skipped: nothing matches, nothing of the chain runs
    got, flops, stats = engine.expand_exists(ctx, np.full(70, SKIP, dtype=U64), L.m, L.dp, L.dm)
    assert not got.any() and flops == 0 and stats[:3] == [0, 0, 0]


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_gives_back_what_it_allocates(ctx, mode, dirty):
    g = OwnershipGraph(ctx)
    try:
        with ctx.options(expand_mode=mode):
            for hops in (1, 2, 3):
                m, dp, dm = g.layers(dirty, hops)
                for lab in (None, g.label):
                    got = held_and_steady(ctx, lambda: engine.expand_exists(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab))
                    rp, _, _ = engine.expand(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab)
                    assert got[0][2] == (np.diff(np.asarray(rp).astype(I64)) > 0).tobytes()
    finally:
        for x in (g.M, g.DP, g.DM):
            x.free()
