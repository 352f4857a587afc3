"""Every form decision of the expand chain's driver (spgemm.hip: expand_device) by name: the result against the oracle, and the
profiler scopes that show the intended path ran, with their launch counts where the hop matters.

The graphs and the cells are those of tests/chain_graph.py: which hop leaves the sorted-CSR form, by push or by scatter, the
scatter's state lazily or fully zeroed, the empty source rows dropped or kept — each read off the graph on the host
(Graph.check_cell runs again here before anything goes to the device).  A row below gives the scopes a cell's expand_mat must
show, with their counts, and the scopes it must not; expand_count swaps the last pull for its counting form.

  gather_rows_kernel                        a sorted-CSR product (one per clean hop; m, dp and dm products over dirty layers)
  first_hop_copy_kernel / fhd_cand_kernel   the clean / dirty first-hop shortcut
  bp_push_csr_kernel<m|dm|dp>               leaving by push        bp_scatter_csr_kernel   leaving by scatter
  cr_build_kernel                           the empty source rows were dropped
  bp_pull_kernel<sparse|dense>              a pulled hop; a lazily zeroed state must meet the sparse one (bp_hop_plan refuses otherwise)

Not reachable by construction, kept here as rows that cannot exist:
  - leaving by push at hop index 2 of std: T2 * 32 <= nnz would need nnz >= 3.2 M on a graph of at most 20 000 vertices whose
    hop-1 cells need nnz == 32 * T1; the push at the last hop of a chain is met by the two-hop boundary cells instead.
  - a lazily zeroed state of more than 56 words: w * 2048 B of checksum tables beside the sparse pull's 48 KiB exceed the LDS,
    bp_from_csr zeroes such a state as a whole (cells "6 k 4095 ..." and wider are "full" for that reason or by |F1| * 8 >= n).
  - expand_count with a checksum over 8192 uncompacted rows: 128 words of tables do not fit the LDS (FGPU_INVALID, "batch the
    sources"); those rows count without the checksum, and the compacted (8192, 4096) cell checks the checksum at 64 words.
"""
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_graph as cg  # noqa: E402

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64

G, FH, FHD = "gather_rows_kernel", "first_hop_copy_kernel", "fhd_cand_kernel"
PM, PDM, PDP = "bp_push_csr_kernel<m>", "bp_push_csr_kernel<dm>", "bp_push_csr_kernel<dp>"
PUSH, SC, CR = "bp_push_csr_kernel*", "bp_scatter_csr_kernel", "cr_build_kernel"
SP, DE, PULLS = "bp_pull_kernel<sparse>", "bp_pull_kernel<dense>", "bp_pull_kernel*"
ROWS_EMIT, PAIRS_FILL, EMIT_SORT = "bp_rows_kernel<emit>", "bp_pairs_kernel<fill>", "emission sort (pairs by row)"
PROBE, PAIRS_OUT = "bp_probe_rows_kernel", "pairs_fill_kernel"

# cell: (launches expand_mat must show, scopes it must not; a trailing * matches every scope that starts so)
ROWS = {
    "1 ratio too small": ({FH: 1, G: 2}, ["bp_*", CR, FHD]),
    "1 mode 1": ({FH: 1, G: 2}, ["bp_*", CR, FHD]),
    "2 T1 * ratio == nnz: stays, leaves at 2, full": ({FH: 1, G: 1, SC: 1, CR: 1, DE: 1}, [SP, PUSH, FHD]),
    "2 T1 * ratio == nnz + 1: leaves at 1, lazy": ({FH: 1, SC: 1, SP: 1, DE: 1}, [G, PUSH, CR]),
    "2 T1 * 32 == nnz: push at 1": ({FH: 1, PM: 1, DE: 1}, [G, SC, CR, SP, PDM, PDP]),
    "2 T1 * 32 == nnz + 1: scatter at 1": ({FH: 1, SC: 1, SP: 1, DE: 1}, [G, PUSH, CR]),
    "2 |F1| * 8 == n: scatter at 1, full": ({FH: 1, SC: 1, DE: 2}, [G, PUSH, CR, SP]),
    "2 leaves at 2, full": ({FH: 1, G: 1, SC: 1, CR: 1, DE: 1}, [SP, PUSH]),
    "2 leaves at 2, lazy": ({FH: 1, G: 1, SC: 1, CR: 1, SP: 1}, [DE, PUSH]),
    "2 dirty, push at 1": ({FHD: 1, PM: 1, PDM: 1, PDP: 1, DE: 1}, [FH, G, SC, CR, SP]),
    "2 dirty, leaves at 2": ({FHD: 1, G: 3, SC: 1, CR: 1, DE: 1}, [FH, SP, PUSH]),
    "3 mode 2, light first hop": ({PM: 1, SP: 1, DE: 1}, [FH, FHD, G, SC, CR]),
    "3 mode 2, heavy first hop": ({SC: 1, CR: 1, SP: 1, DE: 2}, [FH, FHD, G, PUSH]),
    "3 mode 0, general first hop": ({PM: 1, SP: 1, DE: 1}, [FH, FHD, G, SC, CR]),
    "4 T by mxm_flops": ({G: 1, PM: 1, DE: 1}, [FH, FHD, SC, CR, SP]),
    "5 hypersparse at 1": ({FH: 1, G: 1, SC: 1, CR: 1, DE: 1}, [SP, PUSH]),
    "7 compacted, scatter at 1": ({FHD: 1, SC: 1, CR: 1, SP: 1, DE: 1}, [FH, G, PUSH]),
    "7 small, compacted, push at 1": ({FHD: 1, PM: 1, PDM: 1, PDP: 1, CR: 1, DE: 1}, [FH, G, SC, SP]),
    # the chain of a three-hop probe: two hops ending in bits, then the probe of the last matrix
    "7 probe, push at 1": ({FH: 1, PM: 1, PROBE: 1}, [G, SC, CR, PULLS]),
    "7 probe, compacted, scatter at 1": ({FHD: 1, SC: 1, CR: 1, SP: 1, PROBE: 1}, [FH, G, PUSH, DE]),
    "7 probe, small, compacted, push at 1": ({FHD: 1, PM: 1, PDM: 1, PDP: 1, CR: 1, PROBE: 1}, [FH, G, SC, PULLS]),
}
PATH_CELLS = [c for c in ROWS if c[0] in "12345"]
# the full cross of the ends: an uncompacted and two compacted chains at n >= 4096, and the ballot transpose below it
END_CELLS = ["2 T1 * 32 == nnz: push at 1", "2 leaves at 2, full", "7 compacted, scatter at 1", "7 small, compacted, push at 1"]
PROBE_CELLS = [c for c in ROWS if c.startswith("7 probe")]


@pytest.fixture(scope="module")
def graphs(ctx):
    extra = []

    def get(cell):
        """The cell's graph, its inequalities asserted once more, and its layers on the device (the hypersparse copy at the
        hop that asks for one)."""
        g = cg.check(cell)
        name, hops, opts, _ = cg.CELLS[cell]
        m, dp, dm = g.device_layers(ctx, hops)
        if "hyper" in opts:
            if not hasattr(g, "_hyper"):
                deg = np.diff(g.a.rowptr.astype(I64))
                rows = np.nonzero(deg)[0].astype(U64)
                short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
                g._hyper = ctx.mat_from_csr(g.n, g.n, short, g.a.colidx, hyper_rows=rows)
                extra.append(g._hyper)
            m = list(m)
            m[opts["hyper"]] = g._hyper
        return g, (m, dp, dm), cg.device_options(opts)

    yield get
    for m in extra:
        m.free()
    for g in cg._made.values():
        g.__dict__.pop("_hyper", None)
        g.free()


def run(ctx, opts, call):
    """call() under exactly these options; its result and the launches by profiler scope."""
    with cg.forced(ctx, **opts):
        ctx.prof_enable(True)
        try:
            out = call()
            launches = {}
            for p in ctx.prof_read():
                launches[p["kernel"]] = launches.get(p["kernel"], 0) + p["launches"]
        finally:
            ctx.prof_enable(False)
    return out, launches


def check_scopes(launches, must, must_not):
    print({k: launches.get(k, 0) for k in must}, sorted(launches))
    for k, c in must.items():
        assert launches.get(k, 0) == c, (k, c, launches)
    for k in must_not:
        hit = [s for s in launches if (s.startswith(k[:-1]) if k.endswith("*") else s == k)]
        assert not hit, (k, hit)


def count_scopes(g, cell, checksum, fuse=1):
    """The row of a cell for expand_count: the last hop counts where its rows are produced (fused), so its pull runs in the
    counting form; a chain whose last hop was the push, and an unfused count, run bp_count_kernel over the final state."""
    must, must_not = ROWS[cell]
    must, must_not = dict(must), list(must_not)
    _, hops, _, path = cg.CELLS[cell]
    if path["leave"] is None:
        return must, must_not
    unfused = "bp_count_kernel<checksum>" if checksum else "bp_count_kernel<count>"
    if not fuse or not path["pulls"]:
        must[unfused] = 1
        return must, must_not + ["bp_pull_kernel<sparse, count>", "bp_pull_kernel<dense, count>"]
    last = SP if path["pulls"][-1] == "sparse" else DE
    must[last] -= 1
    if not must[last]:
        del must[last]
        must_not.append(last)
    form = g.count_pull(hops, path["leave"], path["compact"], checksum)
    must["bp_pull_kernel<%s, count>" % form] = 1
    must_not += ["bp_pull_kernel<%s, count>" % ("dense" if form == "sparse" else "sparse"), "bp_count_kernel<checksum>",
                 "bp_count_kernel<count>"]
    return must, must_not


def export(m):
    rp, ci, _ = m.export_csr()
    m.free()
    return np.asarray(rp).astype(U64), np.asarray(ci).astype(U64)


def assert_csr(rp, ci, want):
    assert np.array_equal(np.asarray(rp).astype(U64), want.rowptr.astype(U64))
    assert np.array_equal(np.asarray(ci).astype(U64), want.colidx.astype(U64))


# ---- cells 1 to 5: the path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", PATH_CELLS)
def test_path_expand_mat(ctx, graphs, cell):
    g, (m, dp, dm), opts = graphs(cell)
    hops = cg.CELLS[cell][1]
    want, want_flops, _ = g.ref(hops)[:3]   # (a hypersparse copy holds the same entries)

    def call():
        out, flops = engine.expand_mat(ctx, g.src, m, dp, dm)
        return export(out) + (flops,)

    (rp, ci, flops), launches = run(ctx, opts, call)
    print(cell, g.figures(), opts)
    assert_csr(rp, ci, want)
    assert flops == want_flops            # (cell 4: the same flops whether T came from the first hop's copy or from mxm_flops)
    check_scopes(launches, *ROWS[cell])


@pytest.mark.parametrize("checksum", [True, False], ids=["checksum", "count"])
@pytest.mark.parametrize("cell", PATH_CELLS)
def test_path_expand_count(ctx, graphs, cell, checksum):
    g, (m, dp, dm), opts = graphs(cell)
    hops = cg.CELLS[cell][1]
    want, want_flops, want_cs = g.ref(hops)[:3]   # (a hypersparse copy holds the same entries)
    got, launches = run(ctx, opts, lambda: engine.expand_count(ctx, g.src, m, dp, dm, want_checksum=checksum))
    assert got == (want.nnz, want_cs if checksum else 0, want_flops), (got, want.nnz, want_cs, want_flops)
    check_scopes(launches, *count_scopes(g, cell, checksum))


def test_every_source_skipped(ctx, graphs):
    """An empty frontier: k empty rows, zero count, zero flops, and nothing of the chain runs."""
    g, (m, dp, dm), opts = graphs("2 T1 * 32 == nnz: push at 1")
    src = np.full(g.k, cg.SKIP, dtype=U64)
    want, want_flops, want_cs = g.ref(3, src=src)[:3]
    assert want.nnz == 0 and want_flops == 0

    def call():
        out, flops = engine.expand_mat(ctx, src, m, dp, dm)
        return export(out) + (flops, engine.expand_count(ctx, src, m, dp, dm))

    (rp, ci, flops, cnt), launches = run(ctx, opts, call)
    assert_csr(rp, ci, want)
    assert len(rp) == g.k + 1 and flops == 0 and cnt == (0, want_cs, 0)
    check_scopes(launches, {}, ["bp_*", CR, FH, FHD, G])


@pytest.mark.parametrize("mode", [0, 2])
def test_empty_matrix_mid_chain(ctx, graphs, mode):
    """[A, empty, A]: the first hop runs (and is counted), the frontier is empty from hop index 1 on."""
    g, (m, dp, dm), opts = graphs("2 T1 * 32 == nnz: push at 1")
    opts = dict(opts, expand_mode=mode)
    e = oracle.empty(g.n, g.n)
    layers = [(g.a, None, None), (e, None, None), (g.a, None, None)]
    want, want_flops, want_cs = g.ref(3, layers=layers)[:3]
    assert want.nnz == 0 and want_flops == g.figures()["T"][0]
    E = ctx.mat_from_csr(g.n, g.n, np.zeros(g.n + 1, dtype=U64), np.zeros(0, dtype=U64))
    try:
        def call():
            out, flops = engine.expand_mat(ctx, g.src, [m[0], E, m[0]])
            return export(out) + (flops, engine.expand_count(ctx, g.src, [m[0], E, m[0]]))

        (rp, ci, flops, cnt), launches = run(ctx, opts, call)
    finally:
        E.free()
    assert_csr(rp, ci, want)
    assert len(rp) == g.k + 1 and flops == want_flops and cnt == (0, want_cs, want_flops)
    if mode == 0:
        check_scopes(launches, {FH: 2}, ["bp_*", CR, G])
    else:
        check_scopes(launches, {PM: 2}, [FH, G, SC, CR])   # (in bit form the later hops run over the empty state)


# ---- cell 6: the (k, nlive) boundaries of the compaction ----------------------------------------------------------------------
@pytest.mark.parametrize("k,nlive", list(cg.BOUNDARY_COMPACTS))
def test_compaction_boundary(ctx, graphs, k, nlive):
    """cr_build_kernel runs exactly where the table says and never under expand_compact=0; the two settings give the same
    matrix, count and checksum (k <= 4095 ranks the rows in one workgroup, from 4096 on by flags and a scan)."""
    results = []
    for compact_opt in (1, 0):
        cell = "6 k %d, live %d, compact %d" % (k, nlive, compact_opt)
        g, (m, dp, dm), opts = graphs(cell)
        path = cg.CELLS[cell][3]
        assert path["compact"] == bool(cg.BOUNDARY_COMPACTS[(k, nlive)] and compact_opt)
        if k > 2048:
            opts = dict(opts, expand_scan_min=0)          # the call stays a batch: the whole-frontier path never compacts
        want, want_flops, want_cs = g.ref(2)[:3]
        must = {FHD: 1} if k < cg.FH_MAX_ROWS else {G: 3}
        must_not = [FH] + ([G] if k < cg.FH_MAX_ROWS else [FHD])
        if path["how"] == "push":
            must.update({PM: 1, PDM: 1, PDP: 1})
            must_not += [SC, PULLS]
        else:
            must[SC] = 1
            must_not += [PUSH]
        if path["compact"]:
            must[CR] = 1
        else:
            must_not.append(CR)
        checksum = k < 8192 or path["compact"]                # (128 words of checksum tables do not fit the LDS: see the docstring)

        def call_mat():
            out, flops = engine.expand_mat(ctx, g.src, m, dp, dm)
            return export(out) + (flops,)

        (rp, ci, flops), launches = run(ctx, opts, call_mat)
        print(cell, g.figures(), opts)
        assert_csr(rp, ci, want)
        assert flops == want_flops
        mm = dict(must)
        if path["pulls"]:
            mm[SP if path["pulls"][0] == "sparse" else DE] = 1
        check_scopes(launches, mm, must_not + ([DE] if path["pulls"] == ("sparse",) else [SP]))
        got, launches = run(ctx, opts, lambda: engine.expand_count(ctx, g.src, m, dp, dm, want_checksum=checksum))
        assert got == (want.nnz, want_cs if checksum else 0, want_flops), (got, want.nnz, want_cs, want_flops)
        mc = dict(must)
        if path["pulls"]:
            mc["bp_pull_kernel<%s, count>" % g.count_pull(2, 1, path["compact"], checksum)] = 1
        else:
            mc["bp_count_kernel<checksum>" if checksum else "bp_count_kernel<count>"] = 1
        check_scopes(launches, mc, must_not)
        results.append((rp, ci, flops, got[0], got[2]))
    for a, b in zip(*results):
        assert np.array_equal(a, b)


# ---- cell 7: the ends ---------------------------------------------------------------------------------------------------------
def chain_row(cell):
    must, must_not = ROWS[cell]
    return dict(must), list(must_not)


@pytest.mark.parametrize("label", [False, True], ids=["", "label"])
@pytest.mark.parametrize("cell", END_CELLS)
def test_end_expand(ctx, graphs, cell, label):
    g, (m, dp, dm), opts = graphs(cell)
    want, want_flops, _ = g.ref(3, label=label)[:3]
    (rp, ci, flops), launches = run(ctx, opts, lambda: engine.expand(ctx, g.src, m, dp, dm, g.label() if label else None))
    assert rp.dtype == U64 and ci.dtype == U64
    assert_csr(rp, ci, want)
    assert flops == want_flops
    check_scopes(launches, *chain_row(cell))


@pytest.mark.parametrize("label", [False, True], ids=["", "label"])
@pytest.mark.parametrize("emit_sort", [0, 2])
@pytest.mark.parametrize("cell", END_CELLS)
def test_end_expand_mat_emission(ctx, graphs, cell, emit_sort, label):
    g, (m, dp, dm), opts = graphs(cell)
    want, want_flops, _ = g.ref(3, label=label)[:3]

    def call():
        out, flops = engine.expand_mat(ctx, g.src, m, dp, dm, g.label() if label else None)
        assert (out.nrows, out.ncols, out.nvals) == (g.k, g.n, want.nnz)
        return export(out) + (flops,)

    (rp, ci, flops), launches = run(ctx, dict(opts, expand_emit_sort=emit_sort), call)
    assert_csr(rp, ci, want)
    assert flops == want_flops
    must, must_not = chain_row(cell)
    if emit_sort == 2 and g.n >= 4096:
        must.update({PAIRS_FILL: 1, EMIT_SORT: 1})
        must_not.append(ROWS_EMIT)
    else:                                  # the ballot transpose: asked for, or the only form below 4096 vertices
        must[ROWS_EMIT] = 1
        must_not += [PAIRS_FILL, EMIT_SORT]
    check_scopes(launches, must, must_not)


@pytest.mark.parametrize("pinned", [False, True], ids=["free", "pinned"])
@pytest.mark.parametrize("row_bits", [16, 32])
@pytest.mark.parametrize("cell", END_CELLS)
def test_end_expand_pairs(ctx, graphs, cell, row_bits, pinned):
    label = row_bits == 16
    g, (m, dp, dm), opts = graphs(cell)
    want, want_flops, _ = g.ref(3, label=label)[:3]
    rows, cols = want.pairs()
    pin = None
    if pinned:
        # a row in three is pinned to one of its destinations, one to a vertex it does not reach, one stays free
        i = np.arange(g.k)
        deg = np.diff(want.rowptr.astype(I64))
        first = want.colidx[np.minimum(want.rowptr[:-1].astype(I64) + deg // 2, max(want.nnz - 1, 0))]
        pin = np.where(i % 3 == 0, np.where(deg > 0, first, U64(g.L0)), np.where(i % 3 == 1, U64(g.L0), cg.SKIP)).astype(U64)
        p = pin[rows.astype(I64)]
        keep = (p == cg.SKIP) | (p == cols)
        assert 0 < keep.sum() < len(keep) and (keep & (p != cg.SKIP)).any()
        rows, cols = rows[keep], cols[keep]
    (r, c, flops), launches = run(ctx, opts, lambda: engine.expand_pairs(ctx, g.src, m, dp, dm, g.label() if label else None,
                                                                         pinned_dest=pin, row_bits=row_bits))
    assert np.array_equal(r, rows) and np.array_equal(c, cols)
    assert flops == want_flops
    must, must_not = chain_row(cell)
    must[PAIRS_OUT] = 1
    check_scopes(launches, must, must_not)


@pytest.mark.parametrize("label", [False, True], ids=["", "label"])
@pytest.mark.parametrize("cell", END_CELLS)
def test_end_expand_stream(ctx, graphs, cell, label):
    """Chunks of 37 rows: no divisor of any k here, so the last chunk is short."""
    g, (m, dp, dm), opts = graphs(cell)
    want, want_flops, _ = g.ref(3, label=label)[:3]
    assert g.k % 37

    def call():
        s = engine.ExpandStream(ctx, g.src, m, dp, dm, g.label() if label else None, chunk_rows=37)
        try:
            got = [(first, np.array(rp, dtype=U64), np.array(d, dtype=U64)) for first, rp, d in s]
            return got, s.nnz, s.flops
        finally:
            s.close()

    (chunks, nnz, flops), launches = run(ctx, opts, call)
    assert nnz == want.nnz and flops == want_flops
    assert [c[0] for c in chunks] == list(range(0, g.k, 37))
    for first, rp, d in chunks:
        nr = min(37, g.k - first)
        assert len(rp) == nr + 1
        base = want.rowptr[first]
        assert np.array_equal(rp + base, want.rowptr[first:first + nr + 1])
        assert np.array_equal(d, want.colidx[int(base):int(want.rowptr[first + nr])])
    check_scopes(launches, *chain_row(cell))


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("checksum", [True, False], ids=["checksum", "count"])
@pytest.mark.parametrize("cell", END_CELLS)
def test_end_expand_count(ctx, graphs, cell, checksum, fuse):
    """With the label bitmap (test_path_expand_count runs without): the count and the row hashes of a compacted chain go
    through rowmap, fused into the last hop or over the final state."""
    g, (m, dp, dm), opts = graphs(cell)
    want, want_flops, want_cs = g.ref(3, label=True)[:3]
    got, launches = run(ctx, dict(opts, expand_fuse_count=fuse),
                        lambda: engine.expand_count(ctx, g.src, m, dp, dm, g.label(), want_checksum=checksum))
    assert got == (want.nnz, want_cs if checksum else 0, want_flops), (got, want.nnz, want_cs, want_flops)
    check_scopes(launches, *count_scopes(g, cell, checksum, fuse))


@pytest.mark.parametrize("label", [False, True], ids=["", "label"])
@pytest.mark.parametrize("cell", PROBE_CELLS)
def test_end_expand_probe(ctx, graphs, cell, label):
    """A three-hop probe: its chain is the cell's two hops ending in bits.  The destinations cover rows that were compacted
    away and skipped sources (asked for a vertex another row reaches), vertices the label drops, ids >= ncols, hits and misses."""
    g, _, opts = graphs(cell)
    m, dp, dm = g.device_layers(ctx, 3)
    full = g.ref(3)[0]
    _, want_flops, _, fr = g.ref(2)
    lab = cg.label_ids(g.n)
    in_label = np.zeros(g.n, dtype=bool)
    in_label[lab] = True
    deg = np.diff(full.rowptr.astype(I64))
    lr = np.flatnonzero(deg > 0)
    i = np.arange(g.k)
    mid = full.colidx[np.minimum(full.rowptr[:-1].astype(I64) + deg // 2, full.nnz - 1)].astype(I64)
    other = np.full(g.k, int(full.row(lr[0])[0]), dtype=I64)                  # what the first live row reaches
    dropped = np.array([next((int(v) for v in full.row(r) if not in_label[int(v)]), int(mid[r])) if deg[r] else int(other[r])
                        for r in range(g.k)], dtype=I64)
    dst = np.select([deg == 0, i % 5 == 0, i % 5 == 1, i % 5 == 2, i % 5 == 3],
                    [other, mid, g.L3 + (i * 7) % 64, g.n + i, dropped], default=mid).astype(U64)
    valid = g.src != cg.SKIP
    ok = valid & (dst < U64(g.n))
    want = np.zeros(g.k, dtype=bool)
    want[ok] = full.has_edges(i[ok], dst[ok])
    if label:
        want &= in_label[np.minimum(dst.astype(I64), g.n - 1)]
    dead = deg == 0
    assert dead[~valid].all() and (dead & valid).any() and want.any() and (~want[~dead]).any() and not want[dead].any()
    assert (dst[valid] >= U64(g.n)).any() and (~in_label[dst[ok].astype(I64)] & full.has_edges(i[ok], dst[ok])).any()
    (got, flops), launches = run(ctx, opts, lambda: engine.expand_probe(ctx, g.src, dst, m, dp, dm, g.label() if label else None))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    assert flops == want_flops
    check_scopes(launches, *chain_row(cell))
