"""The XCD-partitioned count hop with direct entries (bitpart.hip, option expand_xp_direct): a (partition, row) run of ONE
entry of A' leaves the stream, and the fold reads that row of X itself instead of a partial row.  Results must be the
oracle's, bit-identical between expand_xp_direct = 0 and 1, and the plan must hold exactly the single-entry runs that a numpy
count over the oracle's CSR finds under the same ranking of the rows of X."""
import numpy as np
import pytest

import oracle
from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64 = np.uint64


def partition_of_rows(a: oracle.CSR):
    """The plan's partition of row u of X: rows ranked by out-degree (descending, ties by id), rank r in partition r % 8."""
    deg = np.diff(a.rowptr.astype(np.int64))
    key = 65535 - np.minimum(deg, 65535)
    by_rank = np.argsort(key, kind="stable")
    rank = np.empty(a.nrows, dtype=np.int64)
    rank[by_rank] = np.arange(a.nrows)
    return rank % 8


def single_entry_runs(a: oracle.CSR) -> int:
    """(destination v, partition k) pairs of A' with exactly one entry: v has one in-neighbour in partition k."""
    rows, cols = a.pairs()
    part = partition_of_rows(a)
    key = cols.astype(np.int64) * 8 + part[rows.astype(np.int64)]
    return int(np.count_nonzero(np.bincount(key, minlength=8 * a.ncols) == 1))


def device(ctx, a: oracle.CSR):
    return ctx.mat_from_csr(a.nrows, a.ncols, a.rowptr, a.colidx)


def Forced(ctx, direct, **extra):
    """The partitioned form on any state size, the bit-parallel chain, the given direct mode (and whole-frontier settings or any
    other option that has a read-back, expand_mode included); what was set before comes back on exit."""
    opts = dict(expand_mode=2, expand_xcd_min_mb=0, expand_xp_direct=direct)
    opts.update(extra)
    return ctx.options(**opts)


# ---- a hand-built graph whose destinations cover every case of the fold ---------------------------------------------------
N = 8192                # 8 partitions of 1024 rows: one in-hub's run in a partition spans two chunks of the stream
D = 16                  # every vertex has out-degree D: ranks are ids, partition(u) = u % 8
HUB = 200               # in-edges from every vertex: a run of 1024 entries in each partition (the zrows path)
BEFORE_HUB, AFTER_HUB = 199, 201   # one in-edge each (partitions 3 and 0), next to the hub's runs
ALL_DIRECT = 300        # one in-neighbour in each of the 8 partitions
ONE_EDGE = 301          # one in-edge in total
DELTA_DM, DELTA_DP = 400, 402      # direct-only destinations a tombstone / a pending add names (the side-buffer path)
MASKED = 500            # direct-only, outside the destination label
SPECIAL = {
    BEFORE_HUB: [3003],
    AFTER_HUB: [4000],
    ALL_DIRECT: [1000 + k for k in range(8)],
    ONE_EDGE: [1234],
    DELTA_DM: [3001, 3010],
    DELTA_DP: [3105],
    MASKED: [5001, 5012],
}


@pytest.fixture(scope="module")
def small_graph():
    rng = np.random.default_rng(0xD1EC7)
    out = {u: {HUB} for u in range(N) if u != HUB}
    out[HUB] = set()
    for v, us in SPECIAL.items():
        for u in us:
            out[u].add(v)
    banned = set(SPECIAL) | {HUB}
    for u in range(N):
        while len(out[u]) < D:
            v = int(rng.integers(0, N))
            if v != u and v not in banned:
                out[u].add(v)
    rows = np.concatenate([np.full(len(out[u]), u, dtype=U64) for u in range(N)])
    cols = np.concatenate([np.array(sorted(out[u]), dtype=U64) for u in range(N)])
    a = oracle.build_csr(N, N, rows, cols)
    assert np.all(np.diff(a.rowptr.astype(np.int64)) == D)
    assert np.array_equal(partition_of_rows(a), np.arange(N) % 8)
    # the cases are what they claim: in-neighbour partitions of each special destination
    at = oracle.transpose(a)
    ins = lambda v: at.colidx[int(at.rowptr[v]):int(at.rowptr[v + 1])].astype(np.int64)
    assert sorted(ins(ALL_DIRECT) % 8) == list(range(8)) and len(ins(ONE_EDGE)) == 1
    assert np.all(np.bincount(ins(HUB) % 8, minlength=8) >= 1023)
    # tombstones: one in-edge of DELTA_DM and a few random entries; pending adds: one into DELTA_DP and a few random ones
    # outside A
    dm_r, dm_c = [3001], [DELTA_DM]
    pr, pc = [77], [DELTA_DP]
    arows, acols = a.pairs()
    for i in rng.choice(len(arows), 40, replace=False):
        dm_r.append(int(arows[i]))
        dm_c.append(int(acols[i]))
    have = set(zip(arows.tolist(), acols.tolist()))
    while len(pr) < 40:
        u, v = int(rng.integers(0, N)), int(rng.integers(0, N))
        if (u, v) not in have and v not in banned:
            pr.append(u)
            pc.append(v)
    assert (77, DELTA_DP) not in have
    dm = oracle.build_csr(N, N, np.array(dm_r, dtype=U64), np.array(dm_c, dtype=U64))
    dp = oracle.build_csr(N, N, np.array(pr, dtype=U64), np.array(pc, dtype=U64))
    label_ids = np.setdiff1d(np.arange(N)[oracle.mix64(np.arange(N, dtype=U64)) % U64(3) != 0], [MASKED])
    label_ids = np.union1d(label_ids, [ALL_DIRECT, ONE_EDGE, AFTER_HUB, BEFORE_HUB, HUB, DELTA_DM, DELTA_DP])
    return a, dp, dm, label_ids


@pytest.mark.parametrize("nsrc", [100, 600])
def test_direct_entries_of_a_hand_built_graph_match_the_oracle(ctx, small_graph, nsrc):
    """Every input of a destination direct, one in-edge in total, direct runs next to an in-hub's multi-chunk runs, direct-only
    destinations named by a tombstone and by a pending add, a destination outside the label: clean and dirty, with and
    without the label, count-only and checksum, in both direct modes (bit rows of 2 and 16 words)."""
    a, dp, dm, label_ids = small_graph
    src = np.arange(0, N, N // nsrc, dtype=U64)[:nsrc]
    src = src[src != HUB]
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    label = oracle.bits_from_ids(N, label_ids)
    refs = {}
    for dirty in (False, True):
        c, flops, _ = oracle.expand_omp(src, [(a, dp, dm) if dirty else (a, None, None)] * 3)
        rows, cols = c.pairs()
        keep = np.isin(cols, label_ids)
        cl = oracle.build_csr(c.nrows, c.ncols, rows[keep], cols[keep])
        refs[dirty] = ((c.nnz, oracle.checksum_omp(c), flops), (cl.nnz, oracle.checksum_omp(cl), flops))
        assert int(np.count_nonzero(cols == MASKED)) > 0 and int(np.count_nonzero(cols == ALL_DIRECT)) > 0
    expect_direct = single_entry_runs(a)
    assert expect_direct > 0
    got = {}
    for direct in (0, 1):
        with Forced(ctx, direct):
            for dirty in (False, True):
                lay = ([A] * 3, [DP] * 3, [DM] * 3) if dirty else ([A] * 3, None, None)
                r = engine.expand_count(ctx, src, *lay)
                assert r == refs[dirty][0], (direct, dirty)
                assert ctx.get_option("expand_xp_last_direct") == (expect_direct if direct else 0), (direct, dirty)
                nn, cs, fl = engine.expand_count(ctx, src, *lay, want_checksum=False)
                assert (nn, fl) == (refs[dirty][0][0], refs[dirty][0][2])
                rl = engine.expand_count(ctx, src, *lay, dst_label_bitmap=label)
                assert rl == refs[dirty][1], (direct, dirty, "label")
                got[(direct, dirty)] = (r, rl)
    assert got[(0, False)] == got[(1, False)] and got[(0, True)] == got[(1, True)]


# ---- RMAT-20 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat20_direct(ctx):
    A = ctx.mat_rmat(20)
    rp, ci, _ = A.export_csr()
    a = oracle.CSR(A.nrows, A.ncols, rp, ci)
    n = a.nrows
    dm = A.sample(0x20E, 1000)
    rng = np.random.default_rng(0x20E)
    k = max(1, A.nvals // 1000)
    raw = ctx.mat_from_coo(n, n, rng.integers(0, n, k, dtype=U64), rng.integers(0, n, k, dtype=U64))
    dp = raw.merge(None, A)
    host = []
    for m in (dp, dm):
        mrp, mci, _ = m.export_csr()
        host.append(oracle.CSR(n, n, mrp, mci))
    ids = np.arange(0, 64 * 640 + 4096, dtype=U64)
    src = ids[oracle.mix64(ids) % U64(16) == 0][:640]
    refs = {}
    for dirty in (False, True):
        c, flops, _ = oracle.expand_omp(src, [(a, host[0], host[1]) if dirty else (a, None, None)] * 3)
        refs[dirty] = (c.nnz, oracle.checksum_omp(c), flops)
        del c
    return A, dp, dm, a, src, refs


@pytest.mark.parametrize("whole_frontier", [False, True])
def test_rmat20_direct_modes_match_the_oracle_and_each_other(ctx, rmat20_direct, whole_frontier):
    """RMAT-20, 640 :P sources, clean and dirty, expand_xp_direct 0 and 1: one call of 16-word bit rows, or the whole-frontier
    form (passes of 256 live rows dealt to the lanes).  The plan of mode 1 holds exactly the numpy count of single-entry
    (partition, row) runs."""
    A, dp, dm, a, src, refs = rmat20_direct
    extra = dict(expand_scan_min=256, expand_scan_rows=256) if whole_frontier else {}
    expect_direct = single_entry_runs(a)
    assert expect_direct > a.nnz // 100
    got = {}
    for direct in (0, 1):
        with Forced(ctx, direct, **extra):
            for dirty in (False, True):
                lay = ([A] * 3, [dp] * 3, [dm] * 3) if dirty else ([A] * 3,)
                got[(direct, dirty)] = engine.expand_count(ctx, src, *lay)
                assert got[(direct, dirty)] == refs[dirty], (direct, dirty)
                assert ctx.get_option("expand_xp_last_direct") == (expect_direct if direct else 0), (direct, dirty)
                if whole_frontier:
                    assert ctx.get_option("expand_scan_last_passes") > 1
    assert got[(0, False)] == got[(1, False)] and got[(0, True)] == got[(1, True)]


def test_direct_mode_option_is_checked(ctx):
    before = ctx.get_option("expand_xp_direct")
    with pytest.raises(Exception):
        ctx.set_option("expand_xp_direct", 2)
    assert ctx.get_option("expand_xp_direct") == before
