"""The count hop's short cut over the top hub's out-rows (bitpart.hip bp_xplan_hub_build, bitexpand.hip bp_hub_rows, spgemm.hip
scan_strong_first).

h = the vertex of largest out-degree (smallest id on a tie).  When the rows out(h) hold at least a quarter of the entries of A',
the count hop's plan keeps a reduced plan beside it from which those rows are gone, and a CLEAN partitioned count hop whose state
holds all nsrc bits in row h runs under it: the rows out(h) are then nsrc ones each, and their share of nnz and of the checksum
comes from closed forms.  The decision is taken on the device's state; a whole-frontier call only orders its sources so that
whole passes pass it.

The graphs are built so that the decision is known in advance: only the vertices u % 4 == 1 have an edge to h, a "strong" source
has one of them among its out-neighbours, a "weak" one has none.  Every result is oracle.expand_summary_omp's triple, exactly,
and every case shows which path ran: the profiler scope xp_hub_rows is opened by the hops that took the short cut and by no
other, xp_stream_kernel by every partitioned hop."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_xp_direct import Forced, device  # noqa: E402

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64

N = 8192
H, H2 = 4, 8                       # the hub; a second vertex that may tie with it (H < H2: the smaller id is the hub)
SCOPE = "xp_hub_rows"


@contextmanager
def launched(ctx):
    """{scope: launches} of the profiled kernels launched inside the block (filled when it ends)."""
    seen = {}
    ctx.prof_enable(True)
    try:
        yield seen
    finally:
        try:
            for p in ctx.prof_read():
                seen[p["kernel"]] = seen.get(p["kernel"], 0) + p["launches"]
        finally:
            ctx.prof_enable(False)


def build(hub_out=None, tie=False, selfloop=False, scan=False, seed=0x4B5):
    """8192 vertices.  H -> `hub_out` (default: every even vertex but itself; with `selfloop` itself too).  u % 4 == 1 ("T"): an
    edge to H and six random ones.  u % 8 == 2: strong sources, an edge to the T vertex u - 1 and five random ones.  u % 8 == 3:
    weak sources, six random edges.  u % 8 in (0, 4): six random edges (weak as well).  Random columns are never T vertices, H
    or H2, so in(H) = T and nobody reaches H2.  `tie`: H2 -> every odd vertex and as many as H has.  Not `scan`: u % 8 in (6, 7)
    are like (2, 3).  `scan`: u % 8 == 6 has ONE edge, to the T vertex 1 + 4 (j % 340), j = u // 8 (classes of three and four
    strong sources), u % 8 == 7 ONE edge to the vertex 16 + 8 (j % 340) (classes of weak sources), and the vertices u % 8 == 4
    from 6144 up have no out-edge at all."""
    rng = np.random.default_rng(seed)
    ids = np.arange(N, dtype=I64)
    non_t = ids[(ids % 4 != 1) & (ids != H) & (ids != H2)]
    rows, cols = [], []

    def add(r, c):
        rows.append(np.asarray(r, dtype=I64))
        cols.append(np.asarray(c, dtype=I64))

    def rand(us, k):
        add(np.repeat(us, k), non_t[rng.integers(0, len(non_t), len(us) * k)])

    t = ids[ids % 4 == 1]
    add(t, np.full(len(t), H))
    rand(t, 6)
    strong = ids[(ids % 8 == 2) | ((ids % 8 == 6) & (not scan))]
    add(strong, strong - 1)
    rand(strong, 5)
    weak = ids[(ids % 8 == 3) | ((ids % 8 == 7) & (not scan))]
    rand(weak, 6)
    other = ids[(ids % 4 == 0) & (ids != H) & (ids != H2)]
    if scan:
        other = other[(other % 8 == 0) | (other < 6144)]
        one_s, one_w = ids[ids % 8 == 6], ids[ids % 8 == 7]
        add(one_s, 1 + 4 * ((one_s // 8) % 340))
        add(one_w, 16 + 8 * ((one_w // 8) % 340))
    rand(other, 6)
    if hub_out is None:
        hub_out = ids[(ids % 2 == 0) & ((ids != H) | selfloop)]
    add(np.full(len(hub_out), H), hub_out)
    if tie:
        odd = ids[ids % 2 == 1][:len(hub_out)]
        add(np.full(len(odd), H2), odd)
    else:
        rand(np.array([H2]), 6)
    a = oracle.build_csr(N, N, np.concatenate(rows).astype(U64), np.concatenate(cols).astype(U64))
    # the graph is what it claims
    deg = np.diff(a.rowptr.astype(I64))
    at = oracle.transpose(a)
    assert int(np.argmax(deg)) == H and deg[H] == len(hub_out) and (deg[H2] == deg[H]) == tie
    assert np.array_equal(np.sort(at.row(H).astype(I64)), np.sort(np.append(t, H)) if selfloop else t)
    assert a.nnz >= 4096
    return a


def hub_share(a):
    """entries of A' in the rows out(H) / all entries"""
    indeg = np.bincount(a.colidx[:a.nnz].astype(I64), minlength=N)
    return indeg[a.row(H).astype(I64)].sum() / a.nnz


def is_strong(a, src):
    at = oracle.transpose(a)
    in_h = np.zeros(N, dtype=bool)
    in_h[at.row(H).astype(I64)] = True
    return np.array([bool(np.any(in_h[a.row(int(s)).astype(I64)])) for s in src])


@pytest.fixture(scope="module")
def hub_graph():
    a = build()
    assert hub_share(a) >= 0.25
    return a


def strong_sources(k):
    ids = np.arange(N, dtype=I64)
    return ids[ids % 8 == 2][:k].astype(U64)


def check(ctx, src, host, dev, scope, tag, direct=1, stream=True, label_ids=None, **options):
    """engine.expand_count, with and without the checksum, against the oracle; the scope ran `scope` times per call (True: at
    least once), the stream kernel as `stream` says."""
    want = oracle.expand_summary_omp(src, host, chunk=1024)[:3]
    kw = {}
    if label_ids is not None:
        c, flops, _ = oracle.expand_omp(src, host)
        rows, cols = c.pairs()
        keep = np.isin(cols, label_ids)
        cl = oracle.build_csr(c.nrows, c.ncols, rows[keep], cols[keep])
        assert (c.nnz, oracle.checksum_omp(c), flops) == want and 0 < cl.nnz < c.nnz
        want, kw = (cl.nnz, oracle.checksum_omp(cl), flops), dict(dst_label_bitmap=oracle.bits_from_ids(N, label_ids))
    with Forced(ctx, direct, **options):
        for cs in (True, False):
            with launched(ctx) as seen:
                got = engine.expand_count(ctx, src, *dev, want_checksum=cs, **kw)
            print(tag, "checksum" if cs else "count", got, want, {k: v for k, v in seen.items() if k.startswith("xp_")})
            assert got == (want if cs else (want[0], 0, want[2])), (tag, cs)
            assert ("xp_stream_kernel" in seen) == stream, (tag, cs, sorted(seen))
            if scope is True:
                assert seen.get(SCOPE, 0) >= 1, (tag, cs, sorted(seen))
            else:
                assert seen.get(SCOPE, 0) == scope, (tag, cs, seen.get(SCOPE, 0))
    return want


# ---- one call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsrc", [128, 256, 512, 1024, 200, 1000])
def test_saturated_pass_takes_the_short_cut(ctx, hub_graph, nsrc):
    """Every source reaches H in two hops: rows of 2, 4, 8 and 16 words (QL 1, 2, 4, 8), and a partial last word (200, 1000)."""
    a = hub_graph
    src = strong_sources(nsrc)
    assert len(src) == nsrc and is_strong(a, src).all()
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 1, ("saturated", nsrc))


@pytest.mark.parametrize("nsrc", [128, 1000])
def test_one_source_short_of_the_hub_runs_the_full_plan(ctx, hub_graph, nsrc):
    a = hub_graph
    src = strong_sources(nsrc)
    src[nsrc // 2] = 3 + 8 * 5                               # a weak source: six random edges, none into T
    assert is_strong(a, src).sum() == nsrc - 1
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 0, ("one short", nsrc))


def test_destination_label_drops_some_of_the_hubs_rows(ctx, hub_graph):
    a = hub_graph
    ids = np.arange(N, dtype=U64)
    label_ids = ids[oracle.mix64(ids) % U64(3) != 0]
    out_h = a.row(H)
    assert 0 < np.isin(out_h, label_ids).sum() < len(out_h)
    src = strong_sources(256)
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 1, "label", label_ids=label_ids)


def test_dirty_count_hop_runs_the_full_plan(ctx, hub_graph):
    """A tombstone on an entry of a hub row and a pending add, at the count hop only."""
    a = hub_graph
    rows, cols = a.pairs()
    k = int(np.nonzero(np.isin(cols, a.row(H)) & (rows != H))[0][7])
    dm = oracle.build_csr(N, N, rows[k:k + 1], cols[k:k + 1])
    assert not a.has_edges([11], [12])[0]
    dp = oracle.build_csr(N, N, np.array([11], dtype=U64), np.array([12], dtype=U64))
    src = strong_sources(256)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    host = [(a, None, None), (a, None, None), (a, dp, dm)]
    check(ctx, src, host, ([A] * 3, [None, None, DP], [None, None, DM]), 0, "dirty count hop")


def test_dirty_hop_0_that_unmakes_a_strong_source_is_refused_on_the_device(ctx, hub_graph):
    """The tombstone removes the one edge that made a source strong: by its rows of A the source still is, row H of the state
    says it is not."""
    a = hub_graph
    src = strong_sources(256)
    s = int(src[100])
    assert a.has_edges([s], [s - 1])[0] and is_strong(a, src).all()
    dm = oracle.build_csr(N, N, np.array([s], dtype=U64), np.array([s - 1], dtype=U64))
    A, DM = device(ctx, a), device(ctx, dm)
    host = [(a, None, dm), (a, None, None), (a, None, None)]
    check(ctx, src, host, ([A] * 3, None, [DM, None, None]), 0, "dirty hop 0")


def test_small_hub_share_builds_no_reduced_plan(ctx):
    a = build(hub_out=np.arange(16, 16 + 2 * 64, 2, dtype=I64), seed=0x4B6)
    assert hub_share(a) < 0.25
    src = strong_sources(256)
    assert is_strong(a, src).all()
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 0, "small share")


def test_tie_goes_to_the_smaller_id_and_the_hub_has_a_self_loop(ctx):
    """H and H2 have the same out-degree.  Every source saturates row H and none reaches H2: the short cut is taken only when the
    hub is H, and H itself is one of its own out-rows."""
    a = build(tie=True, selfloop=True, seed=0x4B7)
    assert a.has_edges([H], [H])[0] and hub_share(a) >= 0.25
    src = strong_sources(512)
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 1, "tie, self-loop")


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("cut", [0, 1])
def test_every_form_of_the_plan(ctx, hub_graph, dense, direct, cut):
    a = hub_graph
    src = strong_sources(512)
    A = device(ctx, a)
    check(ctx, src, [(a, None, None)] * 3, ([A] * 3,), 1, ("forms", dense, direct, cut), direct=direct, expand_xp_dense=dense,
          expand_xp_cut=cut)


# ---- whole-frontier calls ---------------------------------------------------------------------------------------------------------
SCAN_KMAX = 5                      # spgemm.hip


def saturated_passes(a, src, pass_rows):
    """The passes of a whole-frontier call that hold strong rows only, as expand_count_scan cuts them: the live sources
    strong-first (stable), the degree-one sources classed by their target — a class of m sources is one row of scale 2^k for
    every set bit k < kmax of m and m >> kmax rows of scale 2^kmax, kmax the value that gives the fewest passes — and every group
    cut into passes of pass_rows rows.  A group lists its rows in live order, so its strong rows come first."""
    deg = np.diff(a.rowptr.astype(I64))[src.astype(I64)]
    live = src[deg > 0].astype(I64)
    strong = is_strong(a, live)
    one = deg[deg > 0] == 1
    target = np.array([int(a.row(int(s))[0]) for s in live[one]], dtype=I64)
    tgt, first, m = np.unique(target, return_index=True, return_counts=True)
    class_strong = strong[one][first]
    nplain, plain_strong = int((~one).sum()), int((strong & ~one).sum())
    bits = [int(((m >> k) & 1).sum()) for k in range(SCAN_KMAX + 1)]
    top = [int((m >> k).sum()) for k in range(SCAN_KMAX + 1)]
    rows_of = lambda kmax: [(0 if k else nplain) + (bits[k] if k < kmax else top[k]) for k in range(kmax + 1)]
    passes_of = lambda kmax: sum(-(-r // pass_rows) for r in rows_of(kmax))
    kmax = min(range(SCAN_KMAX + 1), key=lambda k: (passes_of(k), k))
    ms = m[class_strong]
    total = sat = scaled = 0
    for k, rows in enumerate(rows_of(kmax)):
        s_rows = (0 if k else plain_strong) + int((((ms >> k) & 1) if k < kmax else (ms >> kmax)).sum())
        assert s_rows < rows                                 # weak rows in every group: no short last pass of strong rows only
        total += -(-rows // pass_rows)
        sat += s_rows // pass_rows
        scaled += s_rows // pass_rows if k else 0
    return total, sat, scaled, len(live)


def test_whole_frontier_call_orders_strong_sources_first(ctx):
    """About 5 000 live sources, strong and weak alternating in id order, dead ones among them, degree-one sources in classes of
    three and four on strong and on weak targets: three lanes, passes of 256 rows.  The oracle's triple, nnz and flops of the
    1024-row calls summed, and as many passes under the scope as the model says — some of them of class rows of scale two."""
    a = build(scan=True, seed=0x4B8)
    assert hub_share(a) >= 0.25
    ids = np.arange(N, dtype=I64)
    src = ids[(ids % 4 != 1) & (ids != H) & (ids != H2) & ((ids % 4 != 0) | (ids < 4096) | (ids >= 6144))].astype(U64)
    total, sat, scaled, nlive = saturated_passes(a, src, 256)
    st = is_strong(a, src)
    assert 4500 < nlive < len(src) and sat >= 4 and scaled >= 1 and np.count_nonzero(st[1:] != st[:-1]) > 1000
    A = device(ctx, a)
    host = [(a, None, None)] * 3
    want = check(ctx, src, host, ([A] * 3,), sat, "whole frontier", expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=3)
    with Forced(ctx, 1, expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=3):
        engine.expand_count(ctx, src, [A] * 3)
        assert ctx.get_option("expand_scan_last_passes") == total and ctx.get_option("expand_scan_last_live") == nlive
    with Forced(ctx, 1):
        parts = [engine.expand_count(ctx, src[i:i + 1024], [A] * 3) for i in range(0, len(src), 1024)]
    assert (sum(p[0] for p in parts), sum(p[2] for p in parts)) == (want[0], want[2])


def test_rmat14_whole_frontier_matches_the_oracle(ctx):
    A = ctx.mat_rmat(14)
    rp, ci, _ = A.export_csr()
    a = oracle.CSR(A.nrows, A.ncols, rp, ci)
    ids = np.arange(0, a.nrows, dtype=U64)
    src = ids[oracle.mix64(ids) % U64(4) == 0]
    want = oracle.expand_summary_omp(src, [(a, None, None)] * 3, chunk=1024)[:3]
    for lanes in (3, 1):
        with Forced(ctx, 1, expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=lanes):
            with launched(ctx) as seen:
                got = engine.expand_count(ctx, src, [A] * 3)
            print("rmat14", lanes, got, want, seen.get(SCOPE, 0), ctx.get_option("expand_scan_last_passes"))
            assert got == want, lanes
