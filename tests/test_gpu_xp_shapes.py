"""The XCD-partitioned count hop (bitpart.hip, driven from bp_hop_impl in bitexpand.hip) away from the shapes its other tests
use: vertex counts that are no multiple of 16, 64 or 128 — the plan is then built WITHOUT a ranking of the rows of X, its
partitions are the eight contiguous ranges u // prange, the last ones short or empty, and the last 64-row group is partial —
short and empty partitions, long stretches of rows of A' without entries, chains over three different relations (the hop before
the count hop writes its state in the layout of the NEXT matrix's plan), a rectangular chain, the relayout of a state in both
directions, and the A/B options expand_xcd_relabel and expand_nt.

Every result is the CPU oracle's, exactly: (nnz, checksum, flops) of engine.expand_count, its count-only form and its labelled
form (the label filter done in numpy on the oracle's result).  And every case shows WHICH path ran: the kernel names of the
context's profiler (xp_stream_kernel = the partitioned form, bp_move_rows_kernel = a relayout) and, for expand_xp_direct = 1, the
plan's number of single-entry (destination, partition) runs against a numpy count under the layout the plan must have."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_xp_direct import Forced, device, single_entry_runs  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
I64 = np.int64


# ---- the plan's layout, in numpy ---------------------------------------------------------------------------------------------
def prange_of(nrows_x: int) -> int:
    """Rows of X per partition: ceil(n / 8) rounded up to 16 rows."""
    return ((nrows_x + 7) // 8 + 15) & ~15


def runs_with_one_entry(a: oracle.CSR, part) -> int:
    """(destination v, partition k) pairs of A' with exactly one entry under the given partition of the rows of X."""
    rows, cols = a.pairs()
    key = cols.astype(I64) * 8 + part[rows.astype(I64)]
    return int(np.count_nonzero(np.bincount(key, minlength=8 * a.ncols) == 1))


def single_entry_runs_unranked(a: oracle.CSR) -> int:
    """The identity-layout twin of test_gpu_xp_direct.single_entry_runs: partition(u) = u // prange, no ranking."""
    return runs_with_one_entry(a, np.arange(a.nrows, dtype=I64) // prange_of(a.nrows))


def expected_direct(a: oracle.CSR, relabel=1) -> int:
    """What a plan over `a` must hold: ranked only when the rows of X are a multiple of 128 (and expand_xcd_relabel is on).
    The count of the OTHER layout (and of partition(u) = u % 8) must differ, or the assertion would not tell them apart."""
    ranked = relabel and a.nrows % 128 == 0
    want, other = single_entry_runs_unranked(a), single_entry_runs(a)
    if ranked:
        want, other = other, want
    assert want > 0 and want != other
    if not ranked:
        assert want != runs_with_one_entry(a, np.arange(a.nrows, dtype=I64) % 8)
    return want


# ---- graphs --------------------------------------------------------------------------------------------------------------------
def fill_random(rng, nrows, need, allowed, avoid=None):
    """need[u] DISTINCT random columns out of `allowed` for every row u (none equal to avoid[u]): (rows, cols)."""
    need = np.broadcast_to(np.asarray(need, dtype=I64), (nrows,))
    width = 3 * int(need.max()) + 16
    cand = allowed[rng.integers(0, len(allowed), (nrows, width))]
    order = np.argsort(cand, axis=1, kind="stable")
    srt = np.take_along_axis(cand, order, axis=1)
    dup = np.zeros(cand.shape, dtype=bool)
    later = np.zeros(cand.shape, dtype=bool)
    later[:, 1:] = srt[:, 1:] == srt[:, :-1]                         # a later copy of an earlier draw (the sort is stable)
    np.put_along_axis(dup, order, later, axis=1)
    if avoid is not None:
        dup |= cand == np.asarray(avoid, dtype=cand.dtype)[:, None]
    rank = np.cumsum(~dup, axis=1)
    keep = ~dup & (rank <= need[:, None])
    assert np.array_equal(keep.sum(axis=1), need)
    rows = np.repeat(np.arange(nrows, dtype=I64), need)
    return rows.astype(U64), cand[keep].astype(U64)


def relation(nrows, ncols, seed, deg_lo, deg_hi, hubs=(), no_out=None, cols_allowed=None):
    """A random relation: every row draws deg_lo .. deg_hi columns (duplicates collapse), rows in `no_out` none at all; each
    (hub, step, phase) adds an in-edge to `hub` from every row u with u % step == phase."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(deg_lo, deg_hi + 1, nrows)
    if no_out is not None:
        deg[no_out] = 0
    rows = np.repeat(np.arange(nrows, dtype=I64), deg)
    if cols_allowed is None:
        cols = rng.integers(0, ncols, len(rows))
    else:
        cols = np.asarray(cols_allowed, dtype=I64)[rng.integers(0, len(cols_allowed), len(rows))]
    for hub, step, phase in hubs:
        us = np.arange(phase, nrows, step, dtype=I64)
        if no_out is not None:
            us = us[deg[us] > 0]
        rows = np.concatenate([rows, us])
        cols = np.concatenate([cols, np.full(len(us), hub, dtype=I64)])
    return oracle.build_csr(nrows, ncols, rows.astype(U64), cols.astype(U64))


def deltas(a: oracle.CSR, seed, k=40, banned=(), dm_first=(), dp_first=()):
    """Small delta layers as the other count-hop tests build them: tombstones = `dm_first` + k random entries of a, pending
    adds = `dp_first` + k random pairs outside a (none into `banned`).  Returns (dp, dm)."""
    rng = np.random.default_rng(seed)
    arows, acols = a.pairs()
    pick = rng.choice(a.nnz, k, replace=False)
    dm_r = np.concatenate([np.array([p[0] for p in dm_first], dtype=U64), arows[pick]])
    dm_c = np.concatenate([np.array([p[1] for p in dm_first], dtype=U64), acols[pick]])
    if len(dm_first):
        assert np.all(a.has_edges([p[0] for p in dm_first], [p[1] for p in dm_first]))
    r, c = rng.integers(0, a.nrows, 64 * k), rng.integers(0, a.ncols, 64 * k)
    ok = ~a.has_edges(r, c) & ~np.isin(c, np.asarray(list(banned), dtype=I64))
    r, c = r[ok][:k], c[ok][:k]
    assert len(r) == k
    if len(dp_first):
        assert not np.any(a.has_edges([p[0] for p in dp_first], [p[1] for p in dp_first]))
    dp_r = np.concatenate([np.array([p[0] for p in dp_first], dtype=U64), r.astype(U64)])
    dp_c = np.concatenate([np.array([p[1] for p in dp_first], dtype=U64), c.astype(U64)])
    return oracle.build_csr(a.nrows, a.ncols, dp_r, dp_c), oracle.build_csr(a.nrows, a.ncols, dm_r, dm_c)


def label_of(n, drop=(), add=()):
    ids = np.arange(n, dtype=U64)
    keep = ids[oracle.mix64(ids) % U64(3) != 0]
    keep = np.setdiff1d(keep, np.asarray(list(drop), dtype=U64))
    return np.union1d(keep, np.asarray(list(add), dtype=U64)).astype(U64)


def sources(n, nsrc, exclude=()):
    """nsrc distinct ids spread over 0 .. n - 1 (minus `exclude`), the last vertex among them."""
    ids = (np.arange(nsrc, dtype=I64) * n) // nsrc
    ids = ids[~np.isin(ids, np.asarray(list(exclude), dtype=I64))]
    ids[-1] = n - 1
    assert len(np.unique(ids)) == len(ids)
    return ids.astype(U64)


# ---- running a case --------------------------------------------------------------------------------------------------------------
@contextmanager
def launched(ctx):
    """The names of the profiled kernels launched inside the block (filled when it ends)."""
    names = set()
    ctx.prof_enable(True)
    try:
        yield names
    finally:
        try:
            names.update(p["kernel"] for p in ctx.prof_read())
        finally:
            ctx.prof_enable(False)


class Refs:
    """The oracle's side of one chain: the result, its (nnz, checksum, flops) and the labelled one's."""

    def __init__(self, src, layers, label_ids, n_first=None):
        self.c, flops, self.hop_nnz = oracle.expand_omp(src, layers, n=n_first)
        rows, cols = self.c.pairs()
        keep = np.isin(cols, label_ids)
        cl = oracle.build_csr(self.c.nrows, self.c.ncols, rows[keep], cols[keep])
        self.full = (self.c.nnz, oracle.checksum_omp(self.c), flops)
        self.lab = (cl.nnz, oracle.checksum_omp(cl), flops)
        self.label_bits = oracle.bits_from_ids(self.c.ncols, label_ids)
        assert 0 < cl.nnz < self.c.nnz
        # vertices that hold bits in the state the LAST hop reads: the count hop is dense from an eighth of its rows up
        if len(layers) > 1:
            f = oracle.expand_omp(src, layers[:-1], n=n_first)[0]
            self.last_frontier = len(np.unique(f.colidx))
        else:
            self.last_frontier = len(np.unique(src))
        self.dense = self.last_frontier * 8 >= layers[-1][0].nrows


def dev_layers(mats, dps=None, dms=None):
    clean = lambda l: None if l is None or all(x is None for x in l) else list(l)
    return list(mats), clean(dps), clean(dms)


def count_forms(ctx, src, dev, refs: Refs, stream, move=None, tag=None):
    """engine.expand_count in its three forms against the oracle, each with its path evidence."""
    m, dp, dm = dev
    got = []
    for kw, want in ((dict(), refs.full), (dict(want_checksum=False), (refs.full[0], 0, refs.full[2])),
                     (dict(dst_label_bitmap=refs.label_bits), refs.lab)):
        with launched(ctx) as names:
            r = engine.expand_count(ctx, src, m, dp, dm, **kw)
        print(tag, sorted(kw), r, want, "stream" if "xp_stream_kernel" in names else "-", "move" if "bp_move_rows_kernel" in names else "-")
        assert r == want, (tag, sorted(kw))
        assert ("xp_stream_kernel" in names) == stream, (tag, sorted(kw), sorted(names))
        if move is not None:
            assert ("bp_move_rows_kernel" in names) == move, (tag, sorted(kw), sorted(names))
        got.append(r)
    return tuple(got)


def both_direct_modes(ctx, src, dev, refs: Refs, direct_want=None, stream=True, move=None, tag=None, **options):
    """The case under expand_xp_direct 0 and 1 (forced as test_gpu_xp_direct does, plus `options`): the oracle's tuples, the
    same in both modes, and in mode 1 the plan's direct entries."""
    assert refs.dense == stream or options.get("expand_mode", 2) != 2, (tag, refs.last_frontier)
    got = {}
    for direct in (0, 1):
        with Forced(ctx, direct, **options):
            got[direct] = count_forms(ctx, src, dev, refs, stream, move, (tag, "direct", direct))
            if stream and direct_want is not None:
                assert ctx.get_option("expand_xp_last_direct") == (direct_want if direct else 0), (tag, direct)
    assert got[0] == got[1], tag
    return got[1]


# ---- off-grid vertex counts, one relation: the hand-made destination catalogue at 8192 + 57 --------------------------------------
CAT_N = 8249            # prange 1040: partitions 0 .. 6 of 1040 rows, partition 7 of 969; the last group holds rows 8192 .. 8248
CAT_PR = 1040
CAT_D = 16
HUB_LO, HUB_HI = 200, 8200          # in-edges from every vertex: a run of ~1040 entries (two chunks) in each partition
ALL_DIRECT_LO, ALL_DIRECT_HI = 300, 8210   # one in-neighbour in each of the 8 partitions
ONE_EDGE, LAST = 301, CAT_N - 1     # one in-edge in total (the last vertex is also a source)
DELTA_DM_LO, DELTA_DM_HI = 400, 8220       # direct-only destinations a tombstone names
DELTA_DP_LO, DELTA_DP_HI = 402, 8222       # ... and a pending add
MASKED_LO, MASKED_HI = 500, 8230    # direct-only, outside the destination label
CAT_SPECIAL = {
    HUB_LO - 1: [3003], HUB_LO + 1: [4000], HUB_HI - 1: [3004], HUB_HI + 1: [7300],   # one in-edge each, next to a hub's runs
    ALL_DIRECT_LO: [500 + CAT_PR * k for k in range(8)],
    ALL_DIRECT_HI: [600 + CAT_PR * k for k in range(8)],
    ONE_EDGE: [1234],
    LAST: [1235],
    DELTA_DM_LO: [3002, 5300],
    DELTA_DM_HI: [3001, 4200],
    DELTA_DP_LO: [3106],
    DELTA_DP_HI: [3105],
    MASKED_LO: [5001, 6400],
    MASKED_HI: [5002, 6401],
}


def build_catalogue():
    n = CAT_N
    assert prange_of(n) == CAT_PR and n % 16 and n % 64 and n % 128
    rng = np.random.default_rng(0x5A9E5)
    fr = [np.arange(n, dtype=I64), np.arange(n, dtype=I64)]
    fc = [np.full(n, HUB_LO, dtype=I64), np.full(n, HUB_HI, dtype=I64)]
    for v, us in CAT_SPECIAL.items():
        fr.append(np.array(us, dtype=I64))
        fc.append(np.full(len(us), v, dtype=I64))
    fr, fc = np.concatenate(fr), np.concatenate(fc)
    self_loop = fr == fc
    fr, fc = fr[~self_loop], fc[~self_loop]
    banned = sorted(set(CAT_SPECIAL) | {HUB_LO, HUB_HI})
    need = CAT_D - np.bincount(fr, minlength=n)
    rr, rc = fill_random(rng, n, need, np.setdiff1d(np.arange(n, dtype=I64), banned), avoid=np.arange(n))
    a = oracle.build_csr(n, n, np.concatenate([fr.astype(U64), rr]), np.concatenate([fc.astype(U64), rc]))
    assert np.all(np.diff(a.rowptr.astype(I64)) == CAT_D)
    # the cases are what they claim: in-neighbour partitions of each special destination
    at = oracle.transpose(a)
    ins = lambda v: at.row(v).astype(I64)
    for v in (ALL_DIRECT_LO, ALL_DIRECT_HI):
        assert sorted(ins(v) // CAT_PR) == list(range(8))
    for v in (DELTA_DM_LO, DELTA_DM_HI, MASKED_LO, MASKED_HI):
        assert len(set(ins(v) // CAT_PR)) == len(ins(v)) == 2
    assert len(ins(ONE_EDGE)) == 1 and len(ins(LAST)) == 1 and len(a.row(LAST)) == CAT_D
    for hub in (HUB_LO, HUB_HI):
        per = np.bincount(ins(hub) // CAT_PR, minlength=8)
        assert np.all(per[:7] >= CAT_PR - 1) and per[7] >= n - 7 * CAT_PR - 1 and per[7] > 768
    assert sum(v >= 8192 for v in banned) >= 8
    dp, dm = deltas(a, 0xCA7, banned=banned, dm_first=[(3001, DELTA_DM_HI), (3002, DELTA_DM_LO)],
                    dp_first=[(77, DELTA_DP_HI), (78, DELTA_DP_LO), (LAST, 8245)])
    label_ids = label_of(n, drop=[MASKED_LO, MASKED_HI], add=[v for v in banned if v not in (MASKED_LO, MASKED_HI)])
    return a, dp, dm, label_ids


@pytest.fixture(scope="module")
def catalogue():
    return build_catalogue()


def cat_sources(nsrc):
    return sources(CAT_N, nsrc, exclude=[HUB_LO, HUB_HI])


@pytest.mark.parametrize("nsrc", [100, 160, 400, 640])
def test_hand_built_destinations_on_8249_vertices(ctx, catalogue, nsrc):
    """The destination catalogue of test_gpu_xp_direct on a vertex count off every grid, the special sources placed by
    u // 1040, half of the special destinations in the last, partial 64-row group (ids >= 8192) and the last vertex both a
    source and a destination: clean and dirty, with and without the label, bit rows of 2, 4, 8 and 16 words.  The plan's direct
    entries are those of the UNRANKED layout."""
    a, dp, dm, label_ids = catalogue
    src = cat_sources(nsrc)
    assert src[-1] == LAST
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    want_direct = expected_direct(a)
    for dirty in (False, True):
        refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * 3, label_ids)
        cols = refs.c.colidx
        for v in (MASKED_LO, MASKED_HI, ALL_DIRECT_LO, ALL_DIRECT_HI, LAST, HUB_HI):
            assert int(np.count_nonzero(cols == v)) > 0, v
        dev = dev_layers([A] * 3, [DP] * 3 if dirty else None, [DM] * 3 if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, tag=("catalogue", nsrc, dirty))


# ---- off-grid vertex counts, random relations -------------------------------------------------------------------------------------
def build_random(n):
    if n == 100_003:
        a = relation(n, n, 0x100003, 12, 20, hubs=[(n - 2, 3, 1), (70_001, 5, 0), (12, 7, 3)])
    else:
        a = relation(n, n, 0x1001, 4, 7, hubs=[(n - 3, 2, 0), (444, 3, 1)])
    assert a.nnz >= 4096 and len(a.row(n - 1)) > 0 and len(oracle.transpose(a).row(n - 1)) > 0
    dp, dm = deltas(a, n)
    return a, dp, dm, label_of(n)


@pytest.fixture(scope="module")
def random_graphs():
    return {n: build_random(n) for n in (100_003, 1000)}


@pytest.mark.parametrize("n,nsrc,hops", [(100_003, 100, 3), (100_003, 640, 3), (1000, 160, 2), (1000, 400, 3), (1000, 640, 2)])
def test_random_relation_on_off_grid_vertex_counts(ctx, random_graphs, n, nsrc, hops):
    """100 003 and 1000 vertices (neither a multiple of 16), a random relation with in-hubs whose runs span many chunks: the
    unranked plan, the partial last group (the last vertex is a source, has in-edges and is a destination of the result)."""
    a, dp, dm, label_ids = random_graphs[n]
    src = sources(n, nsrc)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    want_direct = expected_direct(a)
    for dirty in (False, True):
        refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * hops, label_ids)
        assert int(np.count_nonzero(refs.c.colidx == n - 1)) > 0
        dev = dev_layers([A] * hops, [DP] * hops if dirty else None, [DM] * hops if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, tag=("random", n, nsrc, hops, dirty))


# ---- short and empty partitions -------------------------------------------------------------------------------------------------
def build_partition_cases():
    out = {}
    # (a) 200 vertices, 8000 entries: prange 32, partition 6 holds rows 192 .. 199, partition 7 none
    n = 200
    assert prange_of(n) == 32
    rng = np.random.default_rng(0x200)
    rows, cols = fill_random(rng, n, 40, np.arange(n, dtype=I64), avoid=np.arange(n))
    a = oracle.build_csr(n, n, rows, cols)
    assert a.nnz == 8000
    out["tiny"] = (a,) + deltas(a, 0x201, k=12) + (label_of(n),)
    # (b) 8249 vertices, no out-edges from ids >= 7280: partition 7 has rows but no entries; (c) the sinks in partition 3
    n = CAT_N
    for name, lo, hi in (("last", 7 * CAT_PR, n), ("middle", 3 * CAT_PR, 4 * CAT_PR)):
        a = relation(n, n, 0xB00 + lo, 10, 18, hubs=[(8195, 3, 0), (3500, 4, 1)], no_out=np.arange(lo, hi))
        deg = np.diff(a.rowptr.astype(I64))
        assert np.all(deg[lo:hi] == 0) and np.all(np.delete(deg, np.arange(lo, hi)) > 0)
        part = np.bincount(a.pairs()[0].astype(I64) // CAT_PR, minlength=8)
        assert part[lo // CAT_PR] == 0 and np.count_nonzero(part) == 7
        assert len(oracle.transpose(a).row(lo + 5)) > 0                  # the sinks are still destinations
        out[name] = (a,) + deltas(a, 0xB01 + lo) + (label_of(n),)
    return out


@pytest.fixture(scope="module")
def partition_cases():
    return build_partition_cases()


@pytest.mark.parametrize("name,nsrc,hops", [("tiny", 100, 2), ("tiny", 160, 3), ("last", 100, 3), ("last", 400, 3), ("middle", 160, 3),
                                            ("middle", 640, 3)])
def test_short_and_empty_partitions(ctx, partition_cases, name, nsrc, hops):
    """A partition of 8 rows next to one of none (200 vertices: the stream kernel's workgroups of partition 7 find no chunk),
    and partitions that have rows of X but no entry of A' — the last one, or one in the middle (the runs and the chunk table of
    the partition after it start where it would have)."""
    a, dp, dm, label_ids = partition_cases[name]
    n = a.nrows
    src = sources(n, nsrc)                                               # (the last vertex is a sink in "last": an empty source row)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    want_direct = expected_direct(a)
    for dirty in (False, True):
        refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * hops, label_ids)
        dev = dev_layers([A] * hops, [DP] * hops if dirty else None, [DM] * hops if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, tag=("partitions", name, nsrc, hops, dirty))


# ---- sparse destinations ------------------------------------------------------------------------------------------------------------
SPARSE_N = 20_011
BAND = (9000, 12_000)


def build_sparse_destinations(last_row_used):
    """Every in-edge lands on the band 9000 .. 11999 or on one of five isolated ids: thousands of consecutive rows of A'
    without entries before, between and after them (the wavefront-wide fill of the run starts, the tails of every partition)."""
    n = SPARSE_N
    isolated = [5, 4000, 16_001, 19_000] + ([n - 1] if last_row_used else [])
    allowed = np.concatenate([np.arange(*BAND, dtype=I64), np.array(isolated, dtype=I64)])
    a = relation(n, n, 0x5BA25E + last_row_used, 10, 14, hubs=[(10_000, 2, 1), (isolated[-1], 9, 4)], cols_allowed=allowed)
    indeg = np.diff(oracle.transpose(a).rowptr.astype(I64))
    assert set(np.nonzero(indeg)[0]) <= set(allowed.tolist()) and all(indeg[v] > 0 for v in isolated)
    assert (indeg[n - 1] > 0) == bool(last_row_used)
    dp, dm = deltas(a, 0x5BA, banned=np.setdiff1d(np.arange(n), allowed))   # (pending adds stay inside the band too)
    return a, dp, dm, label_of(n, add=isolated)


@pytest.fixture(scope="module")
def sparse_destinations():
    return {used: build_sparse_destinations(used) for used in (0, 1)}


@pytest.mark.parametrize("last_row_used", [0, 1])
@pytest.mark.parametrize("nsrc", [100, 400])
def test_destinations_confined_to_a_band(ctx, sparse_destinations, nsrc, last_row_used):
    a, dp, dm, label_ids = sparse_destinations[last_row_used]
    n = a.nrows
    src = sources(n, nsrc)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    want_direct = expected_direct(a)
    for dirty in (False, True):
        refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * 3, label_ids)
        dev = dev_layers([A] * 3, [DP] * 3 if dirty else None, [DM] * 3 if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, tag=("band", nsrc, last_row_used, dirty))


# ---- chains over different relations ----------------------------------------------------------------------------------------------
GRID_N = 16_384          # a multiple of 128: the plans are ranked, and perm of one relation is not perm of another


def build_three_relations(n):
    rel = {
        "A": relation(n, n, 0xA0 + n, 10, 18, hubs=[(n - 1, 3, 0), (n // 2 + 1, 4, 1)]),
        "B": relation(n, n, 0xB0 + n, 6, 10, hubs=[(n - 5, 2, 1), (17, 5, 2), (n // 3, 6, 0)]),
        "C": relation(n, n, 0xC0 + n, 14, 22, hubs=[(n - 2, 4, 3), (n // 4 + 3, 3, 2)]),
    }
    out = {}
    for k, (name, a) in enumerate(rel.items()):
        assert a.nnz >= 4096
        out[name] = (a,) + deltas(a, 0xD0 + k + n)
    if n % 128 == 0:   # the rankings differ: a state written in B's order is not in C's
        deg = lambda a: np.diff(a.rowptr.astype(I64))
        assert not np.array_equal(np.argsort(-deg(rel["B"]), kind="stable"), np.argsort(-deg(rel["C"]), kind="stable"))
    return out, label_of(n)


@pytest.fixture(scope="module")
def three_relations():
    return {n: build_three_relations(n) for n in (100_003, GRID_N)}


def chain_layers(rel, order, dirty_hops):
    return [(rel[r][0], rel[r][1], rel[r][2]) if h in dirty_hops else (rel[r][0], None, None) for h, r in enumerate(order)]


@pytest.mark.parametrize("n", [100_003, GRID_N])
@pytest.mark.parametrize("order,nsrc,dirty_hops", [
    ("ABC", 160, ()), ("ABC", 640, (0, 1, 2)), ("ABC", 400, (1,)), ("ABC", 640, (2,)),
    ("CAA", 640, ()), ("CAA", 160, (0, 1, 2)), ("CAA", 100, (1,)), ("CAA", 400, (0,)),
])
def test_chains_over_three_relations(ctx, three_relations, n, order, nsrc, dirty_hops):
    """(a)-[:R1]->()-[:R2]->()-[:R3]->(c): the hop over the second relation writes its state in the layout of the THIRD one's
    plan, which the count hop then gathers from — at 16 384 vertices each relation has a ranking of its own, at 100 003 none
    has.  Dirty layers on every hop, on none, or on one hop only.  In the bit-parallel chain the state arrives in the plan's
    order: no relayout runs."""
    rel, label_ids = three_relations[n]
    src = sources(n, nsrc)
    mats = {r: tuple(device(ctx, x) for x in rel[r]) for r in set(order)}
    layers = chain_layers(rel, order, dirty_hops)
    refs = Refs(src, layers, label_ids)
    dev = dev_layers([mats[r][0] for r in order], [mats[r][1] if h in dirty_hops else None for h, r in enumerate(order)],
                     [mats[r][2] if h in dirty_hops else None for h, r in enumerate(order)])
    both_direct_modes(ctx, src, dev, refs, expected_direct(rel[order[-1]][0]), move=False, tag=("chain", n, order, nsrc, dirty_hops))


def build_rectangular(n2):
    n1, n3 = 6007, 10_007
    a = relation(n1, n2, 0x4EC7 + n2, 12, 20, hubs=[(n2 - 1, 3, 0)])
    b = relation(n2, n3, 0x4EC8 + n2, 8, 14, hubs=[(n3 - 1, 2, 1), (4321, 5, 0)])
    return (a,) + deltas(a, 0x4EC9), (b,) + deltas(b, 0x4ECA), label_of(n3)


@pytest.fixture(scope="module")
def rectangular():
    return {n2: build_rectangular(n2) for n2 in (CAT_N, 8192)}


@pytest.mark.parametrize("n2", [CAT_N, 8192])
@pytest.mark.parametrize("nsrc", [160, 640])
def test_rectangular_two_hop_chain(ctx, rectangular, n2, nsrc):
    """A is 6007 x n2, B is n2 x 10 007: the state the count hop reads has n2 rows (unranked at 8249, ranked at 8192), its
    destinations are B's 10 007 columns, and the sources are ids of A's 6007 rows."""
    ra, rb, label_ids = rectangular[n2]
    src = sources(ra[0].nrows, nsrc)
    da, db = tuple(device(ctx, x) for x in ra), tuple(device(ctx, x) for x in rb)
    want_direct = expected_direct(rb[0])
    # (a pushed first frontier lies in vertex order: the ranked plan at 8192 has it moved, the unranked one has nothing to move)
    move = n2 % 128 == 0 and first_hop_is_pushed(src, ra[0])
    assert move == (n2 == 8192 and nsrc == 160)
    for dirty in (False, True):
        layers = [ra, rb] if dirty else [(ra[0], None, None), (rb[0], None, None)]
        refs = Refs(src, layers, label_ids, n_first=ra[0].nrows)
        assert refs.c.ncols == rb[0].ncols
        dev = dev_layers([da[0], db[0]], [da[1], db[1]] if dirty else None, [da[2], db[2]] if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, move=move, tag=("rectangular", n2, nsrc, dirty))


# ---- relayout, both directions ------------------------------------------------------------------------------------------------------
def build_grid_regular():
    """16 384 vertices of out-degree exactly 16 (and two in-hubs)."""
    n = GRID_N
    rng = np.random.default_rng(0x6E1D)
    hubs = np.array([n - 1, 5000], dtype=I64)
    fr = np.concatenate([np.arange(0, n, 3, dtype=I64), np.arange(1, n, 4, dtype=I64)])
    fc = np.concatenate([np.full(len(range(0, n, 3)), hubs[0], dtype=I64), np.full(len(range(1, n, 4)), hubs[1], dtype=I64)])
    ok = fr != fc
    fr, fc = fr[ok], fc[ok]
    need = 16 - np.bincount(fr, minlength=n)
    rr, rc = fill_random(rng, n, need, np.setdiff1d(np.arange(n, dtype=I64), hubs), avoid=np.arange(n))
    a = oracle.build_csr(n, n, np.concatenate([fr.astype(U64), rr]), np.concatenate([fc.astype(U64), rc]))
    assert np.all(np.diff(a.rowptr.astype(I64)) == 16)
    return (a,) + deltas(a, 0x6E1E) + (label_of(n),)


@pytest.fixture(scope="module")
def grid_regular():
    return build_grid_regular()


@pytest.mark.parametrize("nsrc", [160, 400, 640])
def test_csr_frontier_is_moved_into_the_plan_order(ctx, grid_regular, nsrc):
    """expand_mode 0 (auto), two hops: the first hop runs on sorted CSR, the chain leaves that form at the count hop through a
    scatter of the frontier in VERTEX order, and the partitioned count hop must first move the rows to the slots its ranked
    plan gathers from (bp_move_rows_kernel) — then xp_stream_kernel runs."""
    a, dp, dm, label_ids = grid_regular
    n = a.nrows
    src = sources(n, nsrc)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    want_direct = expected_direct(a)
    for dirty in (False, True):
        refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * 2, label_ids)
        f1 = refs.hop_nnz[0]
        T = 16 * f1                                                      # traversed edges of the last hop over the base matrix
        assert T * 28 > a.nnz and T * 32 > a.nnz                         # it leaves the CSR form, and by the scatter (not the push)
        assert f1 * 8 >= n and min(f1, n) * 8 >= n                       # the scattered state is not lazy, the count hop dense
        dev = dev_layers([A] * 2, [DP] * 2 if dirty else None, [DM] * 2 if dirty else None)
        both_direct_modes(ctx, src, dev, refs, want_direct, move=True, tag=("csr -> plan", nsrc, dirty), expand_mode=0)


def build_funnel():
    """A -> B -> C on 16 384 vertices where B's columns are 1400 ids: the hop over B writes its state in the order of C's plan,
    but the count hop over C then finds fewer than n / 8 rows with bits and takes the sparse pull, in vertex order."""
    n = GRID_N
    funnel = np.arange(3, n, 11, dtype=I64)[:1400]
    assert len(funnel) * 8 < n
    a = relation(n, n, 0xF0A, 10, 14, hubs=[(n - 1, 3, 0)])
    b = relation(n, n, 0xF0B, 8, 12, hubs=[(int(funnel[700]), 2, 0)], cols_allowed=funnel)
    c = relation(n, n, 0xF0C, 10, 16, hubs=[(n - 3, 3, 1), (2222, 4, 0)])
    assert c.nnz >= 4096
    return [(m,) + deltas(m, 0xF10 + k) for k, m in enumerate((a, b, c))], label_of(n)


@pytest.fixture(scope="module")
def funnel():
    return build_funnel()


@pytest.mark.parametrize("nsrc", [100, 160, 400, 640])
def test_state_in_plan_order_is_moved_back_for_the_sparse_pull(ctx, funnel, nsrc):
    rel, label_ids = funnel
    n = GRID_N
    src = sources(n, nsrc)
    mats = [tuple(device(ctx, x) for x in r) for r in rel]
    for dirty in (False, True):
        layers = [r if dirty else (r[0], None, None) for r in rel]
        refs = Refs(src, layers, label_ids)
        assert not refs.dense and refs.last_frontier > 1000
        dev = dev_layers([m[0] for m in mats], [m[1] for m in mats] if dirty else None, [m[2] for m in mats] if dirty else None)
        both_direct_modes(ctx, src, dev, refs, None, stream=False, move=True, tag=("plan -> vertex order", nsrc, dirty))


# ---- a ranked plan whose range is no power of two, states large enough to be recycled ----------------------------------------------
BIG_GRID_N = 65_664      # 513 x 128: ranked, range 8208; 16-word rows make a state of 2^20 words and more, which the chain hands
                         # back to the pool with its non-zero rows cleared IN THE LAYOUT IT WAS WRITTEN IN instead of a memset


@pytest.fixture(scope="module")
def big_relations():
    return build_three_relations(BIG_GRID_N)


def test_ranked_chains_reuse_each_others_recycled_states(ctx, big_relations):
    """Chains over different relations and DIFFERENT sources one after the other on 65 664 vertices: each finds the block the
    one before cleared row by row through its own perm.  A row cleared at the wrong slot would leave the earlier chain's bits
    behind, and the next chain — other sources, another relation's ranking — would count them."""
    rel, label_ids = big_relations
    n = BIG_GRID_N
    assert n % 128 == 0 and n & (n - 1) and prange_of(n) * 8 == n
    mats = {r: tuple(device(ctx, x) for x in rel[r]) for r in "ABC"}
    first, second = sources(n, 640), (sources(n, 640) + U64(7)) % U64(n)
    plan = [("ABC", first, ()), ("CAA", second, (1,)), ("ABC", second, (0, 1, 2)), ("CAB", first, ()), ("ABC", first, ())]
    for order, src, dirty_hops in plan:
        refs = Refs(src, chain_layers(rel, order, dirty_hops), label_ids)
        # the state the count hop read is cleared row by row when under 7 / 8 of its rows are flagged (flagged >= non-zero), else
        # released as it is: both happen in this sequence
        assert n * 16 >= 1 << 20 and not n * 6 <= refs.last_frontier * 8 <= n * 7
        rezero = refs.last_frontier * 8 < n * 6
        dev = dev_layers([mats[r][0] for r in order], [mats[r][1] if h in dirty_hops else None for h, r in enumerate(order)],
                         [mats[r][2] if h in dirty_hops else None for h, r in enumerate(order)])
        with Forced(ctx, 1):
            with launched(ctx) as names:
                assert engine.expand_count(ctx, src, *dev) == refs.full, (order, dirty_hops)
            assert "xp_stream_kernel" in names and "bp_move_rows_kernel" not in names, sorted(names)
            assert ("bp_rezero_rows_kernel" in names) == rezero, (order, sorted(names))
        both_direct_modes(ctx, src, dev, refs, expected_direct(rel[order[-1]][0]), move=False, tag=("recycled", order, dirty_hops))


# ---- bit rows the partitioned form does not take ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100_003, GRID_N])
@pytest.mark.parametrize("nsrc", [50, 1100])
def test_row_widths_outside_the_form_take_the_plain_pull(ctx, three_relations, n, nsrc):
    """One-word rows (50 sources) and 32-word rows (1100 sources): neither the count hop nor the hop before it may use a plan —
    a state written in plan order for a count hop that then reads vertex order would show as a relayout, or as a wrong count."""
    rel, label_ids = three_relations[n]
    src = sources(n, nsrc)
    mats = {r: tuple(device(ctx, x) for x in rel[r]) for r in "ABC"}
    refs = Refs(src, chain_layers(rel, "ABC", (1, 2)), label_ids)
    dev = dev_layers([mats[r][0] for r in "ABC"], [None, mats["B"][1], mats["C"][1]], [None, mats["B"][2], mats["C"][2]])
    for direct in (0, 1):
        with Forced(ctx, direct):
            count_forms(ctx, src, dev, refs, False, move=False, tag=("width", n, nsrc, direct))


# ---- the A/B options ------------------------------------------------------------------------------------------------------------------
def first_hop_is_pushed(src, a: oracle.CSR) -> bool:
    """expand_mode 2: a first frontier whose traversed edges are under a 32nd of the matrix is pushed into the bit state — in
    vertex order, whatever the next hop's plan wants."""
    deg = np.diff(a.rowptr.astype(I64))
    return int(deg[src.astype(I64)].sum()) * 32 <= a.nnz


@pytest.mark.parametrize("order,nsrc", [("ABC", 400), ("CAA", 160), ("AA", 400)])
def test_relabel_off_and_on_agree(ctx, three_relations, order, nsrc):
    """expand_xcd_relabel 1 (ranked plans) and 0 (vertex order) on a multiple-of-128 graph: the oracle's tuples from both, the
    ranked count of direct entries under 1 and the identity-layout count under 0.  The matrices are uploaded afresh for each
    setting — a plan stays with its snapshot.  The two-hop chain pushes its first frontier into a state in vertex order: moved
    under 1, left alone under 0."""
    rel, label_ids = three_relations[GRID_N]
    src = sources(GRID_N, nsrc)
    layers = chain_layers(rel, order, (0, 1, 2))
    refs = Refs(src, layers, label_ids)
    last = rel[order[-1]][0]
    moved = len(order) == 2 and first_hop_is_pushed(src, rel[order[0]][0])
    assert moved == (len(order) == 2)
    got = {}
    for relabel in (1, 0):
        mats = {r: tuple(device(ctx, x) for x in rel[r]) for r in set(order)}
        dev = dev_layers([mats[r][0] for r in order], [mats[r][1] for r in order], [mats[r][2] for r in order])
        got[relabel] = both_direct_modes(ctx, src, dev, refs, expected_direct(last, relabel), move=bool(relabel and moved),
                                         tag=("relabel", relabel, order, nsrc), expand_xcd_relabel=relabel)
    assert got[0] == got[1]


def test_streaming_hints_do_not_change_the_result(ctx, catalogue):
    """expand_nt: bits 1 and 2 pick the non-temporal store / load variants of xp_stream_kernel, bit 4 the fold's loads."""
    a, dp, dm, label_ids = catalogue
    src = cat_sources(400)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    refs = Refs(src, [(a, dp, dm)] * 3, label_ids)
    dev = dev_layers([A] * 3, [DP] * 3, [DM] * 3)
    want_direct = expected_direct(a)
    got = [both_direct_modes(ctx, src, dev, refs, want_direct, tag=("nt", nt), expand_nt=nt) for nt in range(8)]
    assert all(g == got[0] for g in got)


@pytest.mark.parametrize("dirty", [False, True])
def test_whole_frontier_form_on_8249_vertices(ctx, catalogue, dirty):
    """640 sources in passes of 256 live rows (4-word bit rows), each pass a partitioned count hop over the unranked plan."""
    a, dp, dm, label_ids = catalogue
    src = cat_sources(640)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    refs = Refs(src, [(a, dp, dm) if dirty else (a, None, None)] * 3, label_ids)
    dev = dev_layers([A] * 3, [DP] * 3 if dirty else None, [DM] * 3 if dirty else None)
    for direct in (0, 1):
        with Forced(ctx, direct, expand_scan_min=256, expand_scan_rows=256):
            count_forms(ctx, src, dev, refs, True, tag=("whole frontier", direct, dirty))
            assert ctx.get_option("expand_scan_last_passes") > 1
            assert ctx.get_option("expand_xp_last_direct") == (expected_direct(a) if direct else 0)


# ---- the emitting forms on the same inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_emitting_forms_give_the_oracles_rows(ctx, catalogue, three_relations, mode):
    """engine.expand (the result itself, not its count) on the off-grid catalogue and on a chain over three relations."""
    a, dp, dm, label_ids = catalogue
    rel, rel_label = three_relations[100_003]
    cases = [(cat_sources(160), [(a, dp, dm)] * 3, label_ids), (sources(100_003, 160), chain_layers(rel, "ABC", (1,)), rel_label),
             (sources(GRID_N, 100), chain_layers(three_relations[GRID_N][0], "CAA", (0, 1, 2)), three_relations[GRID_N][1])]
    with Forced(ctx, 1, expand_mode=mode):
        for src, layers, lab in cases:
            c, flops, _ = oracle.expand_omp(src, layers)
            dev = dev_layers([device(ctx, l[0]) for l in layers], [device(ctx, l[1]) if l[1] is not None else None for l in layers],
                             [device(ctx, l[2]) if l[2] is not None else None for l in layers])
            rowptr, dest, fl = engine.expand(ctx, src, *dev)
            assert fl == flops
            np.testing.assert_array_equal(rowptr, c.rowptr)
            np.testing.assert_array_equal(dest, c.colidx)
            rows, cols = c.pairs()
            keep = np.isin(cols, lab)
            cl = oracle.build_csr(c.nrows, c.ncols, rows[keep], cols[keep])
            rowptr, dest, fl = engine.expand(ctx, src, *dev, dst_label_bitmap=oracle.bits_from_ids(c.ncols, lab))
            np.testing.assert_array_equal(rowptr, cl.rowptr)
            np.testing.assert_array_equal(dest, cl.colidx)
