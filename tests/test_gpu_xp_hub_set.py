"""The count hop's second reduced plan, for the tier of hubs under the top one (bitpart.hip bp_xplan_hub_set_build, bitexpand.hip
bp_hub_rows, spgemm.hip scan_strong_first).

H = the rows with at least a quarter of the top hub's out-degree, at most 32, by (degree descending, id ascending).  When the rows
of the union of out(H[i]) outside out(H[0]) hold at least an eighth of the entries of A', the plan keeps a second reduced plan
from which the whole union is gone, and a CLEAN partitioned count hop whose state holds all nsrc bits in the row of EVERY hub of H
runs under it.  One that saturates the top hub's row alone runs under the first reduced plan, as before.

The graphs are built so that the decision is known in advance.  Below 8192, the vertices u % 4 == 1 ("T") are the only
in-neighbours of the hubs: T vertex number j has an edge to the hubs of `mids[j % len(mids)]`, a source u % 4 == 2 has ONE
T vertex among its out-neighbours, u - 1, and every other vertex has none.  Every result is oracle.expand_summary_omp's triple,
exactly, and every case shows which path ran: the profiler scope xp_hub_rows is opened by every hop that took a short cut,
xp_hub_set by those that ran under the second plan as well, xp_stream_kernel by every partitioned hop."""
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xp_hub_set_model as model  # noqa: E402
from test_gpu_xp_direct import Forced, device  # noqa: E402
from test_gpu_xp_hub import launched  # noqa: E402

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64

NB = 8192                          # the regular part; the vertices from NB up are the special cases of `build`
N = NB + 8
H1 = 4                             # the top hub: out-edges to every even vertex below NB but itself, 4095 of them
QUARTER = 1024                     # ceil(4095 / 4)
ODD = np.arange(3, NB, 4, dtype=I64)   # the 2048 vertices u % 4 == 3: what the secondary hubs point at
ROWS, SET = "xp_hub_rows", "xp_hub_set"
ALL = "all"


def window(first, count):
    return ODD[first:first + count]


# the default set: three secondary hubs that share out-neighbours (their windows overlap), 8 points at the hub 12 and at 16, 12 has
# a self-loop — and 8, 12, 16, all even, are out-neighbours of H1 as well
HUBS = {8: np.concatenate([window(0, 1100), [12, 16]]), 12: np.concatenate([window(600, 1100), [12]]), 16: window(900, 1100)}


def build(hubs=None, mids=(ALL,), scan=False, seed=0x5E7):
    """N vertices.  H1 -> every even vertex below NB but itself; `hubs`: {secondary hub: its out-neighbours} (ids u % 4 == 0).
    T vertex 1 + 4 j: an edge to every hub of mids[j % len(mids)] (ALL: H1 and every secondary hub) and six random ones.
    u % 4 == 2: sources, an edge to the T vertex u - 1 and five random ones.  u % 4 in (0, 3), hubs aside: six random edges.
    Random columns are never T vertices or hubs, so in(h) is what `mids` says.
    `scan` (with three `mids`): u % 4 == 3 has ONE edge — source number j = u // 4, of kind j % 4, to a T vertex whose number is
    0, 0, 1, 2 modulo 3 for the kinds 0 .. 3, the 512 sources of a kind in 170 classes of three (two of four) per target — and the
    vertices u % 8 == 4 from 6144 up have no out-edge at all.
    From NB up: NB + 1 (T-like) -> every hub but the LAST secondary one, NB + 2 -> NB + 1 and five random; NB + 5 -> every
    secondary hub but not H1, NB + 6 -> NB + 5 and five random; the others have no edge."""
    hubs = HUBS if hubs is None else hubs
    rng = np.random.default_rng(seed)
    ids = np.arange(NB, dtype=I64)
    every = [H1] + sorted(hubs)
    is_hub = np.isin(ids, every)
    non_t = ids[(ids % 4 != 1) & ~is_hub]
    rows, cols = [], []

    def add(r, c):
        rows.append(np.asarray(r, dtype=I64))
        cols.append(np.asarray(c, dtype=I64))

    def rand(us, k):
        add(np.repeat(us, k), non_t[rng.integers(0, len(non_t), len(us) * k)])

    t = ids[ids % 4 == 1]
    for k, mid in enumerate(mids):
        mine = t[np.arange(len(t)) % len(mids) == k]
        for h in (every if mid == ALL else mid):
            add(mine, np.full(len(mine), h))
    rand(t, 6)
    srcs = ids[ids % 4 == 2]
    add(srcs, srcs - 1)
    rand(srcs, 5)
    other = ids[(ids % 4 == 0) & ~is_hub]
    if scan:
        other = other[(other % 8 == 0) | (other < 6144)]
        one = ids[ids % 4 == 3]
        j = one // 4
        kind, c = j % 4, (j // 4) % 170
        add(one, 1 + 4 * (3 * (c + 170 * (kind == 1)) + np.array([0, 0, 1, 2])[kind]))
    else:
        rand(ids[ids % 4 == 3], 6)
    rand(other, 6)
    add(np.full(NB // 2 - 1, H1), ids[(ids % 2 == 0) & (ids != H1)])
    for h, out in hubs.items():
        add(np.full(len(out), h), out)
    add(np.full(len(every) - 1, NB + 1), every[:-1])
    add([NB + 2], [NB + 1])
    rand(np.array([NB + 2]), 5)
    add(np.full(len(every) - 1, NB + 5), every[1:])
    add([NB + 6], [NB + 5])
    rand(np.array([NB + 6]), 5)
    a = oracle.build_csr(N, N, np.concatenate(rows).astype(U64), np.concatenate(cols).astype(U64))
    deg = model.out_degrees(a)
    assert int(np.argmax(deg)) == H1 and deg[H1] == NB // 2 - 1 and -(-int(deg[H1]) // 4) == QUARTER
    assert all(deg[h] == len(np.unique(out)) for h, out in hubs.items()) and a.nnz >= 4096
    return a


class Graph:
    def __init__(self, **kw):
        self.a = build(**kw)
        self.at = oracle.transpose(self.a)
        self.hubs = model.hub_set(self.a)
        self.levels = model.levels(self.a)
        self.union = model.union_rows(self.a, self.hubs)

    def tiers(self, src, hubs=None):
        return model.tiers(self.a, self.at, src, self.hubs if hubs is None else hubs)


@pytest.fixture(scope="module")
def g():
    g = Graph()
    assert g.hubs[0] == H1 and sorted(g.hubs) == [4, 8, 12, 16] and g.levels == 2
    first, extra = model.shares(g.a, g.hubs)
    assert first >= 0.25 and extra >= 0.125
    return g


def sources(k, every=1, phase=0):
    """the first k sources u % 4 == 2 whose T vertex is number j with j % every == phase"""
    ids = np.arange(NB, dtype=I64)
    s = ids[ids % 4 == 2]
    return s[(s // 4) % every == phase][:k].astype(U64)


def check(ctx, src, host, dev, rows, deep, tag, direct=1, stream=True, label_ids=None, **options):
    """engine.expand_count, with and without the checksum, against the oracle; xp_hub_rows ran `rows` times per call and
    xp_hub_set `deep` times, the stream kernel as `stream` says."""
    want = oracle.expand_summary_omp(src, host, chunk=1024)[:3]
    kw = {}
    if label_ids is not None:
        c, flops, _ = oracle.expand_omp(src, host)
        r, cols = c.pairs()
        keep = np.isin(cols, label_ids)
        cl = oracle.build_csr(c.nrows, c.ncols, r[keep], cols[keep])
        assert (c.nnz, oracle.checksum_omp(c), flops) == want and 0 < cl.nnz < c.nnz
        want, kw = (cl.nnz, oracle.checksum_omp(cl), flops), dict(dst_label_bitmap=oracle.bits_from_ids(N, label_ids))
    with Forced(ctx, direct, **options):
        for cs in (True, False):
            with launched(ctx) as seen:
                got = engine.expand_count(ctx, src, *dev, want_checksum=cs, **kw)
            print(tag, "checksum" if cs else "count", got, want, {k: v for k, v in seen.items() if k.startswith("xp_")})
            assert got == (want if cs else (want[0], 0, want[2])), (tag, cs)
            assert ("xp_stream_kernel" in seen) == stream, (tag, cs, sorted(seen))
            assert (seen.get(ROWS, 0), seen.get(SET, 0)) == (rows, deep), (tag, cs, seen.get(ROWS, 0), seen.get(SET, 0))
    return want


def clean(a):
    return [(a, None, None)] * 3


# ---- one call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsrc", [128, 200, 1000, 1024])
def test_all_hubs_saturated_runs_under_the_second_plan(ctx, g, nsrc):
    """Every source reaches every hub of H in two hops: full words (128, 1024) and a partial last word (200, 1000)."""
    src = sources(nsrc)
    assert len(src) == nsrc and (g.tiers(src) == 2).all()
    A = device(ctx, g.a)
    check(ctx, src, clean(g.a), ([A] * 3,), 1, 1, ("all saturated", nsrc))


@pytest.mark.parametrize("nsrc", [128, 1000])
def test_one_source_short_of_one_secondary_hub_runs_under_the_first_plan(ctx, g, nsrc):
    src = sources(nsrc)
    src[nsrc // 2] = NB + 2                                  # reaches H1, 8 and 12, not 16
    assert list(g.tiers(src[nsrc // 2:nsrc // 2 + 1], hubs=g.hubs[:-1])) == [2]
    tier = g.tiers(src)
    assert (tier == 2).sum() == nsrc - 1 and tier[nsrc // 2] == 1
    A = device(ctx, g.a)
    check(ctx, src, clean(g.a), ([A] * 3,), 1, 0, ("one short of a secondary hub", nsrc))


@pytest.mark.parametrize("nsrc", [128, 1000])
def test_one_source_short_of_the_top_hub_runs_the_full_plan(ctx, g, nsrc):
    src = sources(nsrc)
    src[nsrc // 2] = NB + 6                                  # reaches 8, 12 and 16, not H1
    assert list(g.tiers(src[nsrc // 2:nsrc // 2 + 1], hubs=g.hubs[1:])) == [2]
    tier = g.tiers(src)
    assert (tier == 2).sum() == nsrc - 1 and tier[nsrc // 2] == 0
    A = device(ctx, g.a)
    check(ctx, src, clean(g.a), ([A] * 3,), 0, 0, ("one short of the top hub", nsrc))


def test_the_union_counts_every_row_once(ctx, g):
    """Hubs share out-neighbours, one is an out-neighbour of another, one has a self-loop: the rows of the union hold
    nsrc x |union| entries of the result, no more."""
    a = g.a
    out = {h: a.row(h).astype(I64) for h in g.hubs}
    assert len(np.intersect1d(out[8], out[12])) > 100 and len(np.intersect1d(out[12], out[16])) > 100
    assert 12 in out[8] and 8 in out[H1] and 12 in out[12]
    assert len(g.union) < sum(len(o) for o in out.values()) and len(g.union) > len(out[H1])
    nsrc = 200
    src = sources(nsrc)
    c, _, _ = oracle.expand_omp(src, clean(a))
    _, cols = c.pairs()
    assert int(np.isin(cols.astype(I64), g.union).sum()) == nsrc * len(g.union)
    A = device(ctx, a)
    check(ctx, src, clean(a), ([A] * 3,), 1, 1, "union")


def test_destination_label_drops_some_rows_of_the_union(ctx, g):
    ids = np.arange(N, dtype=U64)
    label_ids = ids[oracle.mix64(ids) % U64(3) != 0]
    extra = np.setdiff1d(g.union, g.a.row(H1).astype(I64))
    assert 0 < np.isin(extra, label_ids).sum() < len(extra)
    A = device(ctx, g.a)
    check(ctx, sources(256), clean(g.a), ([A] * 3,), 1, 1, "label", label_ids=label_ids)
    src = sources(256)
    src[7] = NB + 2
    check(ctx, src, clean(g.a), ([A] * 3,), 1, 0, "label, first plan", label_ids=label_ids)


def test_dirty_count_hop_runs_the_full_plan(ctx, g):
    """A tombstone on an entry of a row of the union and a pending add, at the count hop only."""
    a = g.a
    rows, cols = a.pairs()
    extra = np.setdiff1d(g.union, a.row(H1).astype(I64))
    k = int(np.nonzero(np.isin(cols, extra) & ~np.isin(rows, g.hubs))[0][7])
    dm = oracle.build_csr(N, N, rows[k:k + 1], cols[k:k + 1])
    assert not a.has_edges([11], [12])[0]
    dp = oracle.build_csr(N, N, np.array([11], dtype=U64), np.array([12], dtype=U64))
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    host = [(a, None, None), (a, None, None), (a, dp, dm)]
    check(ctx, sources(256), host, ([A] * 3, [None, None, DP], [None, None, DM]), 0, 0, "dirty count hop")


def test_dirty_hop_0_that_unmakes_a_tier_a_source_is_refused_on_the_device(ctx, g):
    """The tombstone removes the one edge that put a source into tier A: by its rows of A the source still is, the hubs' rows of
    the state say it is not."""
    a = g.a
    src = sources(256)
    s = int(src[100])
    assert a.has_edges([s], [s - 1])[0] and (g.tiers(src) == 2).all()
    dm = oracle.build_csr(N, N, np.array([s], dtype=U64), np.array([s - 1], dtype=U64))
    A, DM = device(ctx, a), device(ctx, dm)
    host = [(a, None, dm), (a, None, None), (a, None, None)]
    check(ctx, src, host, ([A] * 3, None, [DM, None, None]), 0, 0, "dirty hop 0")


# ---- the set's edges --------------------------------------------------------------------------------------------------------------
def test_a_row_at_the_quarter_is_in_the_set_and_one_below_is_out(ctx):
    """Hub 12 has exactly ceil(deg(H1) / 4) entries, hub 16 one fewer.  Sources that reach H1, 8 and 12 but not 16 saturate the
    set; sources that reach H1, 8 and 16 but not 12 do not."""
    hubs = {8: window(0, 1100), 12: window(500, QUARTER), 16: window(1000, QUARTER - 1)}
    g = Graph(hubs=hubs, mids=((H1, 8, 12), (H1, 8, 16)), seed=0x5E8)
    assert g.hubs == [H1, 8, 12] and g.levels == 2
    A = device(ctx, g.a)
    for phase, deep in ((0, 1), (1, 0)):
        src = sources(200, every=2, phase=phase)
        assert len(src) == 200 and (g.tiers(src) == (2 if deep else 1)).all()
        check(ctx, src, clean(g.a), ([A] * 3,), 1, deep, ("quarter", phase))


def test_of_more_than_32_rows_the_largest_are_taken_and_the_smaller_id_on_a_tie(ctx):
    """34 qualifying rows: H1, 29 secondary hubs of 1100 entries, one of 1090, two of 1060 (ids 128 < 132) and one of 1040: 128 is
    the 32nd, 132 and 136 are out.  A pass that saturates the 32 but neither 132 nor 136 runs under the second plan; one that
    saturates 132 in the place of 128 does not."""
    ids = [8 + 4 * i for i in range(33)]
    hubs = {h: window(28 * i, 1100) for i, h in enumerate(ids[:29])}
    hubs[ids[29]] = window(900, 1090)
    hubs[ids[30]] = window(920, 1060)
    hubs[ids[31]] = window(940, 1060)
    hubs[ids[32]] = window(960, 1040)
    assert ids[30:] == [128, 132, 136]
    taken = [H1] + ids[:31]
    g = Graph(hubs=hubs, mids=(tuple(taken), tuple([H1] + ids[:30] + [132])), seed=0x5E9)
    assert len(g.hubs) == 32 and g.hubs == taken and g.levels == 2
    assert (model.out_degrees(g.a) >= QUARTER).sum() == 34
    A = device(ctx, g.a)
    for phase, deep in ((0, 1), (1, 0)):
        src = sources(200, every=2, phase=phase)
        assert (g.tiers(src) == (2 if deep else 1)).all()
        check(ctx, src, clean(g.a), ([A] * 3,), 1, deep, ("33rd row", phase))


def test_a_small_extra_share_builds_no_second_plan(ctx):
    """The secondary hubs point at rows that H1 points at already, and at 64 others: the union's extra rows hold far under an
    eighth of the entries, and the first reduced plan works as it did."""
    even = np.arange(20, NB, 2, dtype=I64)
    hubs = {8: np.concatenate([even[:1100], window(0, 64)]), 12: np.concatenate([even[500:1600], window(32, 64)])}
    g = Graph(hubs=hubs, seed=0x5EA)
    assert g.hubs == [H1, 8, 12] and g.levels == 1 and 0 < model.shares(g.a, g.hubs)[1] < 0.125
    src = sources(256)
    assert (g.tiers(src) == 2).all()
    A = device(ctx, g.a)
    check(ctx, src, clean(g.a), ([A] * 3,), 1, 0, "small extra share")


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("cut", [0, 1])
def test_every_form_of_the_plan(ctx, g, dense, direct, cut):
    A = device(ctx, g.a)
    check(ctx, sources(512), clean(g.a), ([A] * 3,), 1, 1, ("forms", dense, direct, cut), direct=direct, expand_xp_dense=dense,
          expand_xp_cut=cut)


# ---- whole-frontier calls ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_case():
    """T vertices take turns: an edge to every hub, to H1 alone, to none — so the sources u % 4 == 2 are of tier A, tier B and weak
    in turn; the vertices u % 4 == 0 (weak) and dead ones lie among them, and the degree-one sources u % 4 == 3 form classes of
    three and four on T vertices of all three kinds."""
    g = Graph(mids=(ALL, (H1,), ()), scan=True, seed=0x5EB)
    assert g.levels == 2 and sorted(g.hubs) == [4, 8, 12, 16]
    ids = np.arange(NB, dtype=I64)
    src = ids[(ids % 4 != 1) & ~np.isin(ids, g.hubs) & ((ids % 4 != 0) | (ids < 4096) | (ids >= 6144))].astype(U64)
    want = oracle.expand_summary_omp(src, clean(g.a), chunk=1024)[:3]
    return g, src, want


@pytest.mark.parametrize("lanes", [3, 1])
def test_whole_frontier_call_orders_tier_a_tier_b_weak(ctx, scan_case, lanes):
    """About 5 000 live sources, passes of 256 rows: the oracle's triple, and as many passes, passes under xp_hub_rows and passes
    under xp_hub_set as the model of the cut says — some of the last of class rows of scale two."""
    g, src, want = scan_case
    total, strong, deep, deep_scaled, nlive = model.tiered_passes(g.a, g.at, src, 256)
    tier = g.tiers(src)
    deg = model.out_degrees(g.a)[src.astype(I64)]
    one = src[deg == 1].astype(I64)
    assert 4500 < nlive < len(src) and deep >= 3 and strong >= deep + 3 and total >= strong + 3 and deep_scaled >= 1
    assert np.count_nonzero(tier[1:] != tier[:-1]) > 1500 and set(np.unique(g.tiers(one))) == {0, 1, 2}
    counts = np.unique(np.array([int(g.a.row(int(s))[0]) for s in one]), return_counts=True)[1]
    assert set(counts) == {3, 4}
    A = device(ctx, g.a)
    opts = dict(expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=lanes)
    got = check(ctx, src, clean(g.a), ([A] * 3,), strong, deep, ("whole frontier", lanes), **opts)
    assert got == want
    with Forced(ctx, 1, **opts):
        engine.expand_count(ctx, src, [A] * 3)
        assert ctx.get_option("expand_scan_last_passes") == total and ctx.get_option("expand_scan_last_live") == nlive


def test_whole_frontier_call_is_the_sum_of_its_1024_row_calls(ctx, scan_case):
    g, src, want = scan_case
    A = device(ctx, g.a)
    with Forced(ctx, 1):
        parts = [engine.expand_count(ctx, src[i:i + 1024], [A] * 3) for i in range(0, len(src), 1024)]
    assert (sum(p[0] for p in parts), sum(p[2] for p in parts)) == (want[0], want[2])


def test_rmat14_whole_frontier_matches_the_oracle(ctx):
    A = ctx.mat_rmat(14)
    rp, ci, _ = A.export_csr()
    a = oracle.CSR(A.nrows, A.ncols, rp, ci)
    ids = np.arange(0, a.nrows, dtype=U64)
    src = ids[oracle.mix64(ids) % U64(4) == 0]
    want = oracle.expand_summary_omp(src, clean(a), chunk=1024)[:3]
    print("rmat14 hub set", model.hub_set(a), "levels", model.levels(a), "shares", model.shares(a, model.hub_set(a)))
    for lanes in (3, 1):
        with Forced(ctx, 1, expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=lanes):
            with launched(ctx) as seen:
                got = engine.expand_count(ctx, src, [A] * 3)
            print("rmat14", lanes, got, want, seen.get(ROWS, 0), seen.get(SET, 0), ctx.get_option("expand_scan_last_passes"))
            assert got == want, lanes
            assert seen.get(SET, 0) <= seen.get(ROWS, 0)
