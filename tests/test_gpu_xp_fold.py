"""The two folds of the XCD-partitioned count hop (bitpart.hip, option expand_xp_fold): 0 = a slot per row and step that loads
all 8 partitions' rows, 1 = a lane per row does the index work and a slot loads each piece (partial row or direct entry) that
exists.  Results must be the oracle's and identical between expand_xp_fold 0 / 1 and expand_xp_direct 0 / 1, on a hand-built
graph whose groups of 64 destinations cover the cases of the piece list and on RMAT-20."""
import numpy as np
import pytest

import oracle
from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64 = np.uint64
I64 = np.int64


def Forced(ctx, fold, direct, **extra):
    """The partitioned form on any state size, the bit-parallel chain, the given fold and direct modes (plus any other option
    that has a read-back), the piece fold at every row width; what was set before comes back on exit."""
    opts = dict(expand_mode=2, expand_xcd_min_mb=0, expand_xp_fold=fold, expand_xp_fold_min_words=2, expand_xp_direct=direct)
    opts.update(extra)
    return ctx.options(**opts)


class Folds:
    """Which fold the calls inside ran, from the context's launch counters: `slot` / `piece` launches since entry."""

    def __init__(self, ctx):
        self.ctx = ctx

    def read(self):
        return self.ctx.get_option("expand_xp_slot_folds"), self.ctx.get_option("expand_xp_piece_folds")

    def __enter__(self):
        self.at = self.read()
        return self

    @property
    def slot(self):
        return self.read()[0] - self.at[0]

    @property
    def piece(self):
        return self.read()[1] - self.at[1]

    def __exit__(self, *exc):
        pass

    def ran_only(self, fold):
        """The partitioned hop ran, and every one of its folds was the kernel of mode `fold`."""
        return (self.slot == 0 and self.piece > 0) if fold else (self.slot > 0 and self.piece == 0)


def device(ctx, a: oracle.CSR):
    return ctx.mat_from_csr(a.nrows, a.ncols, a.rowptr, a.colidx)


MODES = [(fold, direct) for fold in (0, 1) for direct in (0, 1)]

# ---- a hand-built graph ----------------------------------------------------------------------------------------------------
N = 8229                # 128 groups of 64 destinations and one of 37; no multiple of 128, so the rows of X keep vertex order
PRANGE = 1040           # rows of X per partition: ceil(N / 8) rounded up to 16 — partition(u) = u // PRANGE
D = 16                  # every vertex has out-degree D
HUB = 5000              # in-edges from every vertex: a run of ~1000 entries in each partition, two stream chunks (XP_SPAN = 768)
G_DIRECT = 16           # group 16 = destinations 1024 .. 1087: exactly one in-neighbour in each partition (512 direct pieces)
G_EMPTY = 17            # group 17: no in-edge at all
G_PARTIAL = 18          # group 18: two in-neighbours in each partition (512 partial pieces)
ONE_EDGE = 2000         # one in-edge in total
DM_DIRECT, DM_PARTIAL = 2100, 2101    # a tombstone names them: in-neighbours 1 + 1 in two partitions / 3 in one partition
DP_DIRECT, DP_PARTIAL = 2200, 2201    # a pending add names them
OUT_DIRECT, OUT_PARTIAL = 2300, 2301  # outside the destination label
SINGLES = {
    ONE_EDGE: [1234],
    DM_DIRECT: [3001, 5500],
    DM_PARTIAL: [3002, 3003, 3004],
    DP_DIRECT: [3105],
    DP_PARTIAL: [4200, 4201],
    OUT_DIRECT: [5001, 7012],
    OUT_PARTIAL: [6001, 6002],
}


def group(g):
    return range(64 * g, 64 * g + 64)


def partition_of(u):
    return np.asarray(u, dtype=I64) // PRANGE


@pytest.fixture(scope="module")
def small_graph():
    rng = np.random.default_rng(0xF01D)
    out = {u: {HUB} for u in range(N) if u != HUB}
    out[HUB] = set()
    special = dict(SINGLES)
    for i, v in enumerate(group(G_DIRECT)):
        special[v] = [k * PRANGE + 100 + i for k in range(8)]
    for i, v in enumerate(group(G_PARTIAL)):
        special[v] = [k * PRANGE + 200 + i for k in range(8)] + [k * PRANGE + 300 + i for k in range(8)]
    for v, us in special.items():
        for u in us:
            out[u].add(v)
    banned = set(special) | {HUB} | set(group(G_EMPTY))
    for u in range(N):
        while len(out[u]) < D:
            v = int(rng.integers(0, N))
            if v != u and v not in banned:
                out[u].add(v)
    rows = np.concatenate([np.full(len(out[u]), u, dtype=U64) for u in range(N)])
    cols = np.concatenate([np.array(sorted(out[u]), dtype=U64) for u in range(N)])
    a = oracle.build_csr(N, N, rows, cols)

    # ---- the graph is what the cases claim, before the device sees it
    assert N % 64 != 0 and N % 128 != 0 and PRANGE == (((N + 7) // 8 + 15) & ~15)
    assert np.all(np.diff(a.rowptr.astype(I64)) == D)
    at = oracle.transpose(a)
    ins = lambda v: at.colidx[int(at.rowptr[v]):int(at.rowptr[v + 1])].astype(I64)
    per_part = lambda v: np.bincount(partition_of(ins(v)), minlength=8)
    assert np.all(per_part(HUB) > 768)                                   # every partition's run spans two stream chunks
    assert all(np.array_equal(per_part(v), np.ones(8, dtype=I64)) for v in group(G_DIRECT))
    assert all(np.all(per_part(v) >= 2) for v in group(G_PARTIAL))
    assert all(len(ins(v)) == 0 for v in group(G_EMPTY))
    indeg = np.diff(at.rowptr.astype(I64))
    assert indeg[64 * (G_EMPTY - 1):64 * G_EMPTY].sum() > 0 and indeg[64 * (G_EMPTY + 1):64 * (G_EMPTY + 2)].sum() > 0
    assert indeg[64 * (N // 64):].sum() > 0                              # the last, partial group has pieces
    assert len(ins(ONE_EDGE)) == 1
    for v in (DM_DIRECT, DP_DIRECT, OUT_DIRECT):
        assert per_part(v).max() == 1                                    # direct-only
    for v in (DM_PARTIAL, DP_PARTIAL, OUT_PARTIAL):
        assert per_part(v)[per_part(v) > 0].min() >= 2                   # partial-only

    # tombstones: one in-edge of each DM_* destination and a few random entries; pending adds: one into each DP_* destination
    # and a few random ones outside A
    dm_r, dm_c = [3001, 3003], [DM_DIRECT, DM_PARTIAL]
    pr, pc = [77, 78], [DP_DIRECT, DP_PARTIAL]
    arows, acols = a.pairs()
    for i in rng.choice(len(arows), 40, replace=False):
        dm_r.append(int(arows[i]))
        dm_c.append(int(acols[i]))
    have = set(zip(arows.tolist(), acols.tolist()))
    assert (77, DP_DIRECT) not in have and (78, DP_PARTIAL) not in have
    while len(pr) < 40:
        u, v = int(rng.integers(0, N)), int(rng.integers(0, N))
        if (u, v) not in have and v not in banned:
            pr.append(u)
            pc.append(v)
    dm = oracle.build_csr(N, N, np.array(dm_r, dtype=U64), np.array(dm_c, dtype=U64))
    dp = oracle.build_csr(N, N, np.array(pr, dtype=U64), np.array(pc, dtype=U64))
    label_ids = np.arange(N)[oracle.mix64(np.arange(N, dtype=U64)) % U64(3) != 0]
    label_ids = np.setdiff1d(label_ids, [OUT_DIRECT, OUT_PARTIAL])
    label_ids = np.union1d(label_ids, [HUB, ONE_EDGE, DM_DIRECT, DM_PARTIAL, DP_DIRECT, DP_PARTIAL, 64 * G_DIRECT, 64 * G_PARTIAL])
    # single-entry (destination, partition) runs under the plan's layout: what expand_xp_direct = 1 must leave out of the stream
    key = acols.astype(I64) * 8 + partition_of(arows)
    ndirect = int(np.count_nonzero(np.bincount(key, minlength=8 * N) == 1))
    assert ndirect >= 512
    return a, dp, dm, label_ids, ndirect


@pytest.mark.parametrize("nsrc", [100, 200, 400, 600])
def test_both_folds_of_a_hand_built_graph_match_the_oracle(ctx, small_graph, nsrc):
    """Bit rows of 2, 4, 8 and 16 words (1, 2, 4 and 8 lanes per row): a group of 512 direct pieces, a group of 512 partial
    pieces, an empty group between two others, a last group of 37 rows, an in-hub over two chunks, one in-edge in total,
    direct-only and partial-only destinations named by a tombstone, by a pending add and outside the label — clean and dirty,
    with and without the label, with the checksum and count-only, under both folds and both direct modes."""
    a, dp, dm, label_ids, ndirect = small_graph
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
        for v in (OUT_DIRECT, OUT_PARTIAL, 64 * G_DIRECT + 5, 64 * G_PARTIAL + 63, N - 1):
            assert int(np.count_nonzero(cols == v)) > 0, v           # the cases are reached
        assert int(np.count_nonzero((cols >= 64 * G_EMPTY) & (cols < 64 * G_EMPTY + 64))) == 0
    got = {}
    for fold, direct in MODES:
        with Forced(ctx, fold, direct), Folds(ctx) as ran:
            for dirty in (False, True):
                lay = ([A] * 3, [DP] * 3, [DM] * 3) if dirty else ([A] * 3, None, None)
                r = engine.expand_count(ctx, src, *lay)
                assert r == refs[dirty][0], (fold, direct, dirty)
                assert ran.ran_only(fold) and ran.slot + ran.piece == 1 + 4 * dirty, (fold, direct, dirty, ran.slot, ran.piece)
                assert ctx.get_option("expand_xp_last_direct") == (ndirect if direct else 0), (fold, direct, dirty)
                nn, _, fl = engine.expand_count(ctx, src, *lay, want_checksum=False)
                assert (nn, fl) == (refs[dirty][0][0], refs[dirty][0][2]), (fold, direct, dirty, "count only")
                rl = engine.expand_count(ctx, src, *lay, dst_label_bitmap=label)
                assert rl == refs[dirty][1], (fold, direct, dirty, "label")
                nl, _, fl = engine.expand_count(ctx, src, *lay, dst_label_bitmap=label, want_checksum=False)
                assert (nl, fl) == (refs[dirty][1][0], refs[dirty][1][2]), (fold, direct, dirty, "label, count only")
                got[(fold, direct, dirty)] = (r, rl)
            assert ran.ran_only(fold) and ran.slot + ran.piece == 8, (fold, direct, ran.slot, ran.piece)
    for dirty in (False, True):
        assert len({got[(fold, direct, dirty)] for fold, direct in MODES}) == 1


# ---- RMAT-20 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat20(ctx):
    A = ctx.mat_rmat(20)
    rp, ci, _ = A.export_csr()
    a = oracle.CSR(A.nrows, A.ncols, rp, ci)
    n = a.nrows
    dm = A.sample(0xF01D, 1000)
    rng = np.random.default_rng(0xF01D)
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
    return A, dp, dm, src, refs


@pytest.mark.parametrize("scan_rows", [0, 256, 1024])
def test_rmat20_both_folds_match_the_oracle_and_each_other(ctx, rmat20, scan_rows):
    """RMAT-20, 640 :P sources, clean and dirty, under both folds and both direct modes: one call of 16-word bit rows
    (scan_rows = 0), or the whole-frontier path in passes of 256 live rows (4-word rows) and of 1024 (one pass, 16-word rows)."""
    A, dp, dm, src, refs = rmat20
    extra = dict(expand_scan_min=1, expand_scan_rows=scan_rows) if scan_rows else {}
    got = {}
    for fold, direct in MODES:
        with Forced(ctx, fold, direct, **extra), Folds(ctx) as ran:
            for dirty in (False, True):
                lay = ([A] * 3, [dp] * 3, [dm] * 3) if dirty else ([A] * 3,)
                got[(fold, direct, dirty)] = engine.expand_count(ctx, src, *lay)
                assert got[(fold, direct, dirty)] == refs[dirty], (fold, direct, dirty)
                assert ctx.get_option("expand_xp_last_direct") > 0 if direct else ctx.get_option("expand_xp_last_direct") == 0
                if scan_rows:
                    passes = ctx.get_option("expand_scan_last_passes")
                    assert passes > 1 if scan_rows == 256 else passes == 1
            assert ran.ran_only(fold), (fold, direct, ran.slot, ran.piece)
    for dirty in (False, True):
        assert len({got[(fold, direct, dirty)] for fold, direct in MODES}) == 1


def test_fold_is_chosen_by_row_width(ctx, small_graph):
    """expand_xp_fold_min_words: with the piece fold on, rows narrower than the bound keep the slot fold (2- and 16-word rows
    against bounds of 2, 8, 16 and 32), with it off no width gets it; the results do not depend on the choice."""
    a, _, _, _, _ = small_graph
    A = device(ctx, a)
    for nsrc, words in ((100, 2), (600, 16)):
        src = np.arange(0, N, N // nsrc, dtype=U64)[:nsrc]
        got = set()
        for fold in (0, 1):
            for bound in (2, 8, 16, 32):
                with Forced(ctx, fold, 1, expand_xp_fold_min_words=bound), Folds(ctx) as ran:
                    got.add(engine.expand_count(ctx, src, [A] * 3))
                    assert ran.ran_only(1 if fold and words >= bound else 0), (nsrc, fold, bound, ran.slot, ran.piece)
        assert len(got) == 1


def test_fold_option_is_checked(ctx):
    before = ctx.get_option("expand_xp_fold")
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_option("expand_xp_fold", bad)
        assert ctx.get_option("expand_xp_fold") == before
    for v in (0, 1, before):
        ctx.set_option("expand_xp_fold", v)
        assert ctx.get_option("expand_xp_fold") == v
    bound = ctx.get_option("expand_xp_fold_min_words")
    for bad in (0, 1, 3, 64):
        with pytest.raises(Exception):
            ctx.set_option("expand_xp_fold_min_words", bad)
        assert ctx.get_option("expand_xp_fold_min_words") == bound
    for v in (2, 4, 8, 16, 32, bound):
        ctx.set_option("expand_xp_fold_min_words", v)
        assert ctx.get_option("expand_xp_fold_min_words") == v
