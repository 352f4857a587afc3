"""GPU: the nine whole-graph procedures that split their rows at HUB_DEG — fgpu_pagerank, fgpu_wcc, fgpu_cdlp, fgpu_harmonic,
fgpu_betweenness, fgpu_msf, fgpu_maxflow, fgpu_sssp, fgpu_sssp_hops — on the cases of tests/algo_edges.py: one graph with rows
of 4095, 4096, 4097, 8191, 8192 and 8193 entries (0, 1, 2, 2, 2 and 3 hub chunks) at lane 0, lane 63 and in the partial last
word, under three active sets (and, for cdlp and msf, its flipped form: the leaves all hubs share at the END of every hub row);
three separately built copies of it (the hub list's row order comes from an atomicAdd) and its
hypersparse form; graphs of 63 .. 129 vertices; and graphs that take 1 .. 2 B + 1 iterations, for the drivers that read their
counters back once per B.

Every comparison is the one the procedure's own file makes, at its tolerance (imported from there): test_gpu_pagerank.compare
(1e-6 relative, or L1 <= 2 tol one iteration apart), test_gpu_hc.check (registers, stats and reach equal, scores within 1e-9),
test_gpu_bc.close (1e-9) with the three directions bit-identical, exact labels for wcc and cdlp, and the exact comparisons of
test_gpu_msf.check, test_gpu_maxflow.solve, test_gpu_sssp.same and test_gpu_sssp_hops.check."""
import os
import sys

import numpy as np
import pytest

import oracle
from oracle import pagerank as opr
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import algo_edges as ae  # noqa: E402
import bc_check  # noqa: E402
import cdlp_check  # noqa: E402
import hc_check  # noqa: E402
import wcc_check  # noqa: E402
from msf_check import bits_of  # noqa: E402
from sssp_check import sssp as sssp_ref  # noqa: E402
from test_gpu_bc import close as bc_close, run_dirs as bc_run_dirs  # noqa: E402
from test_gpu_cdlp import check as cdlp_check_gpu  # noqa: E402
from test_gpu_hc import check as hc_check_gpu  # noqa: E402
from test_gpu_maxflow import solve as mf_solve  # noqa: E402
from test_gpu_msf import check as msf_check_gpu  # noqa: E402
from test_gpu_pagerank import compare as pr_compare  # noqa: E402
from test_gpu_sssp import same as sssp_same  # noqa: E402
from test_gpu_sssp_hops import check as hops_check  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
B = ae.BATCH
N = ae.LADDER_N
HUBS = np.array(ae.LADDER_HUBS)
DEGS = ae.LADDER_DEGS
MASKS = [m[0] for m in ae.ladder_masks()]
SSSP_AUTO = 4096
SSSP_WIDTHS = (-30, SSSP_AUTO, 1023)          # test_gpu_sssp.test_deterministic_under_every_bucket_width's
BC_SOURCES = (0, 63, 300, 256 + 4096, N - 1)
SSSP_SOURCES = (63, ae.LEAF0 + 97, 1)         # a hub (lane 63), a leaf that points back, the head of the short rows
DEFAULTS = {"pagerank_parts": 1, "wcc_mode": 0, "bc_direction": 0, "bc_batch": 0, "sssp_delta_log2": SSSP_AUTO,
            "maxflow_global_every": 0}
_ref = {}                                     # the checkers' answers, computed once per (procedure, graph, mask)


def ref(key, make):
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def coo(ctx, n, rows, cols, vals=None):
    return ctx.mat_from_coo(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64),
                            None if vals is None else np.asarray(vals, dtype=U64))


def hypersparse(ctx, m):
    """The same entries stored as a delta layer stores them: the ids of the non-empty rows + a row-pointer array over those."""
    rp, ci, vv = m.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(m.nrows, m.ncols, short, ci, vv, hyper_rows=rows)   # (vv is None for a BOOL snapshot)


def builds(ctx, n, rows, cols, vals=None):
    """three snapshots of the same entries: two builds of the sorted COO and one of a shuffled COO.  The hub list of each is
    filled in the order an atomicAdd hands out."""
    shuf = ae.shuffled(rows, cols) if vals is None else ae.shuffled(rows, cols, vals)
    return [coo(ctx, n, rows, cols, vals), coo(ctx, n, rows, cols, vals), coo(ctx, n, *shuf)]


class Ladder:
    def __init__(self, ctx, direction, flip=False):
        self.n, self.rows, self.cols = ae.hub_ladder(direction, flip)
        self.mats = builds(ctx, self.n, self.rows, self.cols)
        self.A = self.mats[0]
        self.Ts = [m.transpose() for m in self.mats]
        self.At = self.Ts[0]
        self.H, self.Ht = hypersparse(ctx, self.A), hypersparse(ctx, self.At)
        self.csr = oracle.build_csr(self.n, self.n, self.rows.astype(U64), self.cols.astype(U64))
        self.rp, self.ci = self.csr.rowptr.astype(np.int64), self.csr.colidx.astype(np.int64)


@pytest.fixture(scope="module")
def ladder(ctx):
    """the ladder's matrices, built once for the module"""
    g = {d: Ladder(ctx, d) for d in ("out", "in", "sym")}
    g["sym-flip"] = Ladder(ctx, "sym", flip=True)             # the shared leaves at the END of every hub row
    return g


@pytest.fixture(autouse=True)
def options_back(ctx):
    yield
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def mask(name):
    """(active or None, clean bitmap or None, dirty bitmap or None, active as bool[n])"""
    _, act, clean, dirty = ae.ladder_masks()[MASKS.index(name)]
    if name == "all":
        return None, None, dirty, act          # (all ones + the bits past n: still every vertex)
    return act, clean, dirty, act


def same_bits(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


# ---- the device holds the ladder --------------------------------------------------------------------------------------------

def test_the_device_snapshots_hold_the_hub_rows(ctx, ladder):
    for d, side in (("out", "A"), ("in", "At"), ("sym", "A"), ("sym-flip", "A")):
        g = ladder[d]
        for m in (g.mats + [g.H] if side == "A" else g.Ts + [g.Ht]):
            rp, ci, _ = m.export_csr()
            deg = np.diff(rp.astype(np.int64))
            assert tuple(deg[HUBS]) == DEGS, (d, side)
            assert np.sort(deg)[-7] < 64                      # six hub rows, every other row short
            assert int(m.nvals) == len(g.rows) <= 75000
            assert not m.has_values
        rp, ci, _ = g.A.export_csr()
        assert np.array_equal(rp.astype(np.int64), g.rp) and np.array_equal(ci.astype(np.int64), g.ci)
    assert N % 64 == 38 and N >= ae.WCC_AUTO_MIN_N            # wcc_mode 0 picks Afforest here


# ---- pagerank -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [0, 2], ids=["one-pass-pull", "xcd-column-ranges"])
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("direction", ["in", "out"])
def test_pagerank_ladder(ctx, ladder, direction, name, parts):
    g = ladder[direction]
    active, clean, dirty, _ = mask(name)
    want, it_ref = ref(("pr", direction, name), lambda: opr.pagerank(g.csr, active=active))
    ctx.set_option("pagerank_parts", parts)
    runs = [engine.pagerank(ctx, g.A, At, bits) for At in (g.At, None) for bits in (clean, dirty)]
    for got, it in runs:
        pr_compare(got, it, want, it_ref)
        assert same_bits((got, it), runs[0])                  # the caller's transpose or the built one, clean or dirty bits
    if active is not None:
        assert (runs[0][0][~active] == 0).all()
    for m in g.mats[1:]:                                       # other builds: the hub partials are summed in chunk order
        assert same_bits(engine.pagerank(ctx, m, None, clean), runs[0])
    for A_, At_ in ((g.H, g.Ht), (g.H, g.At), (g.A, g.Ht), (g.H, None)):
        assert same_bits(engine.pagerank(ctx, A_, At_, clean), runs[0])


@pytest.mark.parametrize("parts", [0, 2], ids=["one-pass-pull", "xcd-column-ranges"])
def test_pagerank_stops_at_every_itermax_around_the_batch(ctx, ladder, parts):
    """tol = 0: the run ends at itermax, wherever that falls in a batch of PR_BATCH blind iterations"""
    g = ladder["in"]
    ctx.set_option("pagerank_parts", parts)
    for L in range(1, 2 * B + 2):
        want, it_ref = ref(("pr-iter", L), lambda: opr.pagerank(g.csr, 0.85, 0.0, L))
        got, it = engine.pagerank(ctx, g.A, g.At, None, 0.85, 0.0, L)
        assert it == it_ref == L
        pr_compare(got, it, want, it_ref, 0.0)


# ---- wcc ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2, 0], ids=["afforest", "full-pass", "auto"])
@pytest.mark.parametrize("name", MASKS)
def test_wcc_ladder(ctx, ladder, name, mode):
    active, clean, dirty, _ = mask(name)
    want = ref(("wcc", name), lambda: wcc_check.wcc_labels(N, ladder["out"].rp, ladder["out"].ci, active))
    ctx.set_option("wcc_mode", mode)
    for d in ("out", "in", "sym"):
        g = ladder[d]
        calls = list(zip(g.mats, g.Ts)) + [(g.H, g.Ht), (g.H, g.At), (g.A, g.Ht)]
        if d == "sym":
            calls += [(m, None) for m in g.mats] + [(g.H, None)]
        for A_, At_ in calls:
            for bits in (clean, dirty):
                got, st = engine.wcc(ctx, A_, At_, bits, stats=True)
                assert np.array_equal(got, want), (d, np.flatnonzero(got != want)[:10])
                assert st[0] == wcc_check.components(want)
        if mode == 2:                                          # the full pass read every entry of the active rows, hub chunks included
            assert engine.wcc(ctx, g.A, g.At, clean, stats=True)[1][1] == int(np.diff(g.rp)[mask(name)[3]].sum())
    assert want[HUBS[mask(name)[3][HUBS]]].max() == want[HUBS[mask(name)[3][HUBS]]].min()   # the active hubs: one component


@pytest.mark.parametrize("mode", [1, 2], ids=["afforest", "full-pass"])
def test_wcc_forest_of_every_depth_around_the_compress_batch(ctx, mode):
    """the path of 2^L + 1 vertices in id order: a chain that pointer jumping halves L times, four jumps per read-back"""
    ctx.set_option("wcc_mode", mode)
    for L, g in ae.batch_paths().items():
        n, rows, cols = g["forest"]
        S = coo(ctx, n, rows, cols)
        D = coo(ctx, n, rows[rows < cols], cols[rows < cols])            # i -> i + 1 only: joined through the transpose
        for A_, At_ in ((S, None), (S, S.transpose()), (D, D.transpose())):
            got, st = engine.wcc(ctx, A_, At_, stats=True)
            assert not got.any() and st[0] == 1, L


# ---- cdlp -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["sym", "sym-flip"])
@pytest.mark.parametrize("name", MASKS)
def test_cdlp_ladder(ctx, ladder, name, form):
    """flipped, the label most of a long row's entries carry after the first iteration (vertex 0's) sits in the row's LAST
    chunks and wins by one vote that only the sum over two chunks gives: 4094 + 1 against 4094"""
    g = ladder[form]
    active, clean, dirty, _ = mask(name)
    rp, ci = cdlp_check.csr_of(N, g.rows, g.cols)
    for itermax in (1, 2, 3, 10):
        want, wst = cdlp_check_gpu(ctx, g.A, N, rp, ci, itermax, active)      # labels and the four counters, entries read included
        for m in g.mats[1:] + [g.H]:
            for bits in (clean, dirty):
                got, st = engine.cdlp(ctx, m, bits, itermax, stats=True)
                assert np.array_equal(got, want) and st == wst, itermax


def test_cdlp_stops_at_every_iteration_around_the_batch(ctx):
    for L, g in ae.batch_paths().items():
        n, rows, cols = g["flood"]
        S = coo(ctx, n, rows, cols)
        rp, ci = cdlp_check.csr_of(n, rows, cols)
        for itermax in sorted({max(L - 1, 0), L, L + 1, 100}):
            want, wst = cdlp_check_gpu(ctx, S, n, rp, ci, itermax)
            assert wst[0] == min(L, itermax)
        assert wst[0] == L and wst[1] == 0 and not want.any()                 # the L-th iteration is the one that changes nothing
        n, rows, cols = g["swap"]
        E = coo(ctx, n, rows, cols)
        rp, ci = cdlp_check.csr_of(n, rows, cols)
        want, wst = cdlp_check_gpu(ctx, E, n, rp, ci, L)
        assert wst[0] == L and want.tolist() == ([1, 0] if L % 2 else [0, 1])  # the labels of parity L


# ---- harmonic -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("direction", ["out", "in"])
def test_harmonic_ladder(ctx, ladder, direction, name):
    g = ladder[direction]
    active, clean, dirty, _ = mask(name)
    rp, ci = hc_check.csr_of(N, g.rows, g.cols)
    score, reach, st = hc_check_gpu(ctx, g.A, ("ladder", direction, name), N, rp, ci, active)
    entries, gathered = ctx.get_option("harmonic_last_entries"), ctx.get_option("harmonic_last_gathered")
    if direction == "out" and name == "all":
        assert entries >= g.A.nvals and gathered >= g.A.nvals                 # the first iteration gathers every entry, the hub chunks' too
    first = engine.harmonic(ctx, g.A, clean, stats=True, registers=True)
    assert same_bits(first[:2], (score, reach)) and first[3] == st
    for m, bits in [(m, clean) for m in g.mats[1:] + [g.H]] + [(g.A, dirty)]:
        assert same_bits(engine.harmonic(ctx, m, bits, stats=True, registers=True), first)


def test_harmonic_stops_at_every_iteration_around_the_batch(ctx):
    for L, g in ae.batch_paths().items():
        n, rows, cols = g["directed"]
        rp, ci = hc_check.csr_of(n, rows, cols)
        score, reach, st = hc_check_gpu(ctx, coo(ctx, n, rows, cols), ("batch", L), n, rp, ci)
        assert st[0] == L and reach[L] == 0


# ---- betweenness ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("direction", ["out", "in"])
def test_betweenness_ladder(ctx, ladder, direction, name):
    g = ladder[direction]
    active, clean, dirty, on = mask(name)
    src = np.array([s for s in BC_SOURCES if on[s]])                          # (a source outside the active set is refused)
    assert len(src) >= 2 and on[0] and 0 in src
    want = ref(("bc", direction, name), lambda: bc_check.betweenness(N, g.rp, g.ci, src, active)[0])
    got, st = bc_run_dirs(ctx, g.A, g.At, src, clean)                         # push, pull and auto: bit-identical
    bc_close(got, want)
    assert st[2] > 0 and got.max() > 0
    for A_, At_, bits in [(m, None, clean) for m in g.mats[1:]] + [(g.A, g.At, dirty), (g.H, g.Ht, clean), (g.H, None, clean),
                                                                   (g.A, g.Ht, clean)]:
        again, st_ = bc_run_dirs(ctx, A_, At_, src, bits)
        assert same_bits(again, got) and st_[3] == st[3]


# ---- msf ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["sym", "sym-flip"])
@pytest.mark.parametrize("kind", ["distinct", "equal"])
def test_msf_ladder(ctx, ladder, kind, form):
    g = ladder[form]
    bits = bits_of(ae.pair_weights(N, g.rows, g.cols, kind))
    Ws = builds(ctx, N, g.rows, g.cols, bits)
    for name in MASKS:
        active, clean, dirty, _ = mask(name)
        st, got = msf_check_gpu(ctx, N, g.rows, g.cols, bits, active, W=Ws[0])
        for W, b in [(W, clean) for W in Ws[1:] + [hypersparse(ctx, Ws[0])]] + [(Ws[0], dirty)]:
            again = engine.msf(ctx, W, b, stats=True)
            assert same_bits(again[:4], got[:4]) and again[4][1] == st[1] and again[4][3] == st[3]
            assert float(again[3].sum()) == float(got[3].sum())               # the total weight
    if kind == "equal":                                                       # BOOL: every weight 1.0, the same pairs
        for name in MASKS:
            active, clean, dirty, on = mask(name)
            st, got = msf_check_gpu(ctx, N, g.rows, g.cols, None, active, W=g.A)
            # one pass per round: the first round read every entry of the active rows, the hub chunks' included
            assert ctx.get_option("msf_last_entries_round0") == int(np.diff(g.rp)[on].sum())
            assert same_bits(engine.msf(ctx, g.H, dirty)[:3], got[:3])


def test_msf_forest_of_every_depth_around_the_compress_batch(ctx):
    """increasing weights along the path of 2^L + 1 vertices: one round hooks every vertex to its smaller neighbour, one
    compress flattens a chain 2^L deep"""
    for L, g in ae.batch_paths().items():
        n, rows, cols = g["forest"]
        bits = bits_of(np.minimum(rows, cols) + 1.0)
        st, got = msf_check_gpu(ctx, n, rows, cols, bits)
        assert st[0] == 1 and not got[0].any() and len(got[1]) == n - 1, L


# ---- maxflow --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True], ids=["hubs-fan-out", "hubs-gather"])
def test_maxflow_ladder(ctx, mirror):
    n, rows, cols, caps, src, sink, hubs = ae.ladder_flow(ae.LADDER_DEGS, mirror)
    Cs = builds(ctx, n, rows, cols, bits_of(caps))
    value, fr, fc, fv, st = mf_solve(ctx, n, rows, cols, caps, src, sink, M=Cs[0])   # certified, and the value is Dinic's
    assert value > 0 and st[0] > 0 and st[3] > 0
    for M in Cs[1:] + [hypersparse(ctx, Cs[0])]:
        again = engine.maxflow(ctx, M, src, sink, stats=True)
        assert again[0] == value and again[4][2] == st[2]


def test_maxflow_pulse_counts_on_both_sides_of_the_batch_and_the_global_relabel(ctx):
    pulses = {}
    for n in range(2, 71):
        rows, cols, caps = ae.bottleneck_path(n)
        value, fr, fc, fv, st = mf_solve(ctx, n, rows, cols, caps, 0, n - 1)
        assert value == 3.25 and len(fr) == n - 1 and np.all(fv == 3.25)
        pulses[n] = st[0]
    print("pulses by path length:", pulses)
    counts = set(pulses.values())
    for edge in (ae.MF_BATCH, ae.MF_GLOBAL_EVERY):                             # a coverage condition on the sweep
        assert min(counts) < edge < max(counts), (edge, sorted(counts))
        assert {c for c in counts if edge - 4 <= c <= edge + 4}, (edge, sorted(counts))


# ---- sssp and sssp_hops ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["distinct", "equal"])
@pytest.mark.parametrize("direction", ["out", "in"])
def test_sssp_ladder(ctx, ladder, direction, kind):
    g = ladder[direction]
    bits = bits_of(ae.pair_weights(N, g.rows, g.cols, kind))
    Ws = builds(ctx, N, g.rows, g.cols, bits)
    H = hypersparse(ctx, Ws[0])
    for src in SSSP_SOURCES:
        want = sssp_ref(N, g.rows, g.cols, bits, src)
        first = None
        for k in SSSP_WIDTHS:
            ctx.set_option("sssp_delta_log2", k)
            got = engine.sssp(ctx, Ws[0], src, stats=True)
            sssp_same(got, want)
            first = first or got
            if direction == "out" and src == 63:
                assert got[2][2] >= 4096                                       # the hub's row was read
        ctx.set_option("sssp_delta_log2", SSSP_AUTO)
        for W in Ws[1:] + [H]:
            again = engine.sssp(ctx, W, src, stats=True)
            assert same_bits(again[:2], first[:2]) and again[2][3] == first[2][3]
    if kind == "equal":                                                       # BOOL: every weight 1.0
        sssp_same(engine.sssp(ctx, g.A, 63, stats=True), sssp_ref(N, g.rows, g.cols, None, 63))


def test_sssp_tight_tree_of_every_depth_around_the_batch(ctx):
    for L, g in ae.batch_paths().items():
        n, rows, cols = g["directed"]
        want = sssp_ref(n, rows, cols, None, 0)
        for vals in (None, bits_of(np.zeros(L))):                              # unit weights; zero weights: one bucket, L levels
            W = coo(ctx, n, rows, cols, vals)
            if vals is not None:
                want = sssp_ref(n, rows, cols, vals, 0)
            for k in SSSP_WIDTHS:
                ctx.set_option("sssp_delta_log2", k)
                got = engine.sssp(ctx, W, 0, stats=True)
                sssp_same(got, want)
                assert got[2][3] == L and got[1][L] == L - 1


@pytest.mark.parametrize("kind", ["distinct", "equal"])
@pytest.mark.parametrize("direction", ["out", "in"])
def test_sssp_hops_ladder(ctx, ladder, direction, kind):
    g = ladder[direction]
    bits = bits_of(ae.pair_weights(N, g.rows, g.cols, kind))
    Ws = builds(ctx, N, g.rows, g.cols, bits)
    H = hypersparse(ctx, Ws[0])
    for src in SSSP_SOURCES:
        table, st = hops_check(ctx, N, g.rows, g.cols, bits, src, 6, W=Ws[0])   # the table's bits and the four counters
        for W in Ws[1:] + [H]:
            again, st_ = engine.sssp_hops(ctx, W, src, 6, stats=True)
            assert same_bits(again, table) and st_ == st


# ---- word edges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ae.WORD_SIZES)
def test_word_graphs(ctx, n):
    rows, cols, masks = ae.word_graphs()[n]
    srows, scols = (x.copy() for x in ae.unique_pairs(n, *ae.sym(rows, cols)))
    A, S = coo(ctx, n, rows, cols), coo(ctx, n, srows, scols)
    At = A.transpose()
    a = oracle.build_csr(n, n, rows.astype(U64), cols.astype(U64))
    rp, ci = a.rowptr.astype(np.int64), a.colidx.astype(np.int64)
    srp, sci = cdlp_check.csr_of(n, srows, scols)
    for name, act, clean, dirty in masks:
        # pagerank, both SpMV forms
        want, it_ref = opr.pagerank(a, active=act)
        for parts in (0, 2):
            ctx.set_option("pagerank_parts", parts)
            got, it = engine.pagerank(ctx, A, At, clean)
            pr_compare(got, it, want, it_ref)
            assert same_bits(engine.pagerank(ctx, A, None, dirty), (got, it))
        # wcc, both modes, with the transpose and as a symmetric pattern
        want = wcc_check.wcc_labels(n, rp, ci, act)
        for mode in (1, 2):
            ctx.set_option("wcc_mode", mode)
            for A_, At_ in ((A, At), (S, None)):
                for bits in (clean, dirty):
                    got, st = engine.wcc(ctx, A_, At_, bits, stats=True)
                    assert np.array_equal(got, want) and st[0] == wcc_check.components(want)
        # cdlp
        for itermax in (1, 10):
            want, wst = cdlp_check_gpu(ctx, S, n, srp, sci, itermax, act)
            got, st = engine.cdlp(ctx, S, dirty, itermax, stats=True)
            assert np.array_equal(got, want) and st == wst
        # harmonic
        score, reach, st = hc_check_gpu(ctx, A, ("word", n, name), n, rp, ci, act)
        assert same_bits(engine.harmonic(ctx, A, dirty, stats=True)[:2], (score, reach))
        # betweenness
        src = np.flatnonzero(act)[[0, 1, -2, -1]]
        got, st = bc_run_dirs(ctx, A, At, src, clean)
        bc_close(got, bc_check.betweenness(n, rp, ci, src, act)[0])
        assert same_bits(bc_run_dirs(ctx, A, None, src, dirty)[0], got)
    # every vertex active
    for parts in (0, 2):
        ctx.set_option("pagerank_parts", parts)
        pr_compare(*engine.pagerank(ctx, A, At), *opr.pagerank(a))
    assert not engine.wcc(ctx, A, At)[0].any()
    cdlp_check_gpu(ctx, S, n, srp, sci, 10)
    hc_check_gpu(ctx, A, ("word", n, "all"), n, rp, ci)
    src = np.array([0, 62 % n, n - 2, n - 1])
    bc_close(bc_run_dirs(ctx, A, At, src)[0], bc_check.betweenness(n, rp, ci, src)[0])


def test_every_option_this_file_touches_is_back_at_its_default(ctx):
    for k, v in DEFAULTS.items():
        assert ctx.get_option(k) == v, k
