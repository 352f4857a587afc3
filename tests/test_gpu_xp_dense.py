"""The fold's groups of the XCD-partitioned count hop (bitpart.hip, option expand_xp_dense): 1 = groups of 64 consecutive RANKS
among the destination rows that have an in-edge in the matrix (nd of them), 0 = groups of 64 consecutive vertex ids.  Results
must be the oracle's and identical between the two forms, under both folds (expand_xp_fold) and both direct modes
(expand_xp_direct), and the get-option expand_xp_last_groups must say which form ran: ceil(nd / 64) or ceil(n / 64).

The hand-built chains are two hops over 8192 vertices: a random relation B of out-degree 16 (so that the state the count hop
reads is dense: well over an eighth of its rows hold bits), then the relation A under test, whose destinations are a chosen set
T — every edge of A ends in T, so nd = |T| exactly.  The delta layers belong to the count hop alone."""
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_xp_fold import Folds, Forced, device  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
I64 = np.int64

N = 8192                # the smallest vertex count at which a relation of one or two entries per row makes a plan (>= 4096 entries)
HOLES = (0, 63, 64, 127, 128, N - 1)
MODES = [(dense, fold, direct) for dense in (0, 1) for fold in (0, 1) for direct in (0, 1)]
WIDTHS = {2: 120, 16: 520}      # words of a bit row: source rows of the call


def destinations(case):
    """T, ascending: the rows of A' that have an entry."""
    if case == "all":
        return np.arange(N, dtype=I64)
    if case == "holes":         # rows without an in-edge exactly at the ends of the first groups of 64 ids, and the first and last vertex
        return np.setdiff1d(np.arange(N, dtype=I64), np.array(HOLES, dtype=I64))
    nd = int(case[2:])
    rng = np.random.default_rng(0xD0 + nd)
    return np.sort(rng.choice(N, nd, replace=False)).astype(I64)


CASES = ["nd1", "nd63", "nd64", "nd65", "nd129", "all", "holes"]


def build_b():
    rng = np.random.default_rng(0xB0B)
    rows = np.repeat(np.arange(N, dtype=U64), 16)
    return oracle.build_csr(N, N, rows, rng.integers(0, N, len(rows)).astype(U64))


class Case:
    """A, its delta layers, the labels and what the plan must count — the graph is what the case claims before the device sees it."""

    def __init__(self, name, b):
        self.name = name
        t = destinations(name)
        nd = self.nd = len(t)
        u = np.arange(N, dtype=I64)
        rows = np.concatenate([u, u])
        cols = np.concatenate([t[(u + 1) % nd], t[(5 * u + 2) % nd]])
        self.a = a = oracle.build_csr(N, N, rows.astype(U64), cols.astype(U64))
        at = oracle.transpose(a)
        indeg = np.diff(at.rowptr.astype(I64))
        assert a.nnz >= 4096 and np.array_equal(np.flatnonzero(indeg), t)
        if name == "nd1":
            assert indeg[t[0]] == N >= 4095 + 1
        if name == "holes":
            assert all(indeg[v] == 0 for v in HOLES) and all(indeg[v] > 0 for v in (1, 62, 65, 126, 129, N - 2))
        if name == "all":
            assert indeg.min() > 0
        self.groups = {0: (N + 63) // 64, 1: (nd + 63) // 64}
        last = t[64 * ((nd - 1) // 64):]                    # the vertices of the last dense group
        assert 1 <= len(last) <= 64 and len(last) == nd - 64 * (self.groups[1] - 1)
        rng = np.random.default_rng(0xDE17A)
        hop1 = b.row(0).astype(I64)                          # vertex 0 is a source of every call: these hold bits in the count hop's state
        # pending adds: into a destination WITHOUT an in-edge in A (none when every row has one), and into rows of T
        empty = np.setdiff1d(np.arange(N, dtype=I64), t)
        self.orphan = int(empty[len(empty) // 2]) if len(empty) else None
        pr, pc = [], []
        if self.orphan is not None:
            pr += hop1.tolist()
            pc += [self.orphan] * len(hop1)
        for x in rng.integers(0, N, 64):
            v = int(t[int(rng.integers(0, nd))])
            if not a.has_edges([int(x)], [v])[0]:
                pr.append(int(x))
                pc.append(v)
        self.dp = oracle.build_csr(N, N, np.array(pr, dtype=U64), np.array(pc, dtype=U64))
        # tombstones: in-edges of the last group's last row and of the first row of T, and a few random entries
        dm_r, dm_c = [], []
        for v in (int(t[-1]), int(t[0])):
            ins = at.row(v).astype(I64)
            for x in ins[:3]:
                dm_r.append(int(x))
                dm_c.append(v)
        arows, acols = a.pairs()
        for i in rng.choice(a.nnz, 40, replace=False):
            dm_r.append(int(arows[i]))
            dm_c.append(int(acols[i]))
        self.dm = oracle.build_csr(N, N, np.array(dm_r, dtype=U64), np.array(dm_c, dtype=U64))
        assert np.all(a.has_edges(dm_r, dm_c)) and int(t[-1]) in last
        ids = np.arange(N, dtype=U64)
        wide = ids[oracle.mix64(ids) % U64(3) != 0].astype(I64)
        if self.orphan is not None:
            wide = np.union1d(wide, [self.orphan])
        self.labels = {"wide": wide, "last group": last}


def reference(case: Case, b, src):
    """{dirty: {form: (nnz, checksum, flops)}} for the full result and each label; the cases are reached."""
    out = {}
    for dirty in (False, True):
        c, flops, hops = oracle.expand_omp(src, [(b, None, None), (case.a, case.dp, case.dm) if dirty else (case.a, None, None)])
        rows, cols = c.pairs()
        res = {"full": (c.nnz, oracle.checksum_omp(c), flops)}
        for tag, ids in case.labels.items():
            mask = np.zeros(N, dtype=bool)
            mask[ids] = True
            keep = mask[cols.astype(I64)]
            cl = oracle.build_csr(c.nrows, c.ncols, rows[keep], cols[keep])
            res[tag] = (cl.nnz, oracle.checksum_omp(cl), flops)
            assert cl.nnz > 0, (case.name, tag)
        if dirty and case.orphan is not None:
            assert int(np.count_nonzero(cols == U64(case.orphan))) > 0       # the row no group holds is reached, by dp alone
        out[dirty] = res
    return out


@pytest.fixture(scope="module")
def relation_b():
    b = build_b()
    # the state the count hop reads is dense for both widths: the rows one hop from the sources are over an eighth of all
    for nsrc in WIDTHS.values():
        f = oracle.expand_omp(sources(nsrc), [(b, None, None)])[0]
        assert len(np.unique(f.colidx[: f.nnz])) * 8 >= N
    return b


def sources(nsrc):
    return ((np.arange(nsrc, dtype=I64) * N) // nsrc).astype(U64)


@pytest.mark.parametrize("words", sorted(WIDTHS))
@pytest.mark.parametrize("name", CASES)
def test_dense_groups_of_a_hand_built_graph_match_the_oracle(ctx, relation_b, name, words):
    """nd = 1, 63, 64, 65, 129, n and n - 6 (no in-edge at ids 0, 63, 64, 127, 128 and n - 1), rows of 2 and 16 words: clean and
    dirty (a pending add into a row without an in-edge in A, a tombstone on a row of the last group), count-only, a wide label
    and a label of the last — partly filled — dense group alone; both group forms, both folds, both direct modes."""
    b = relation_b
    case = Case(name, b)
    src = sources(WIDTHS[words])
    assert src[0] == 0 and words // 2 < (len(src) + 63) // 64 <= words          # (a bit row is a power of two of words)
    refs = reference(case, b, src)
    B, A, DP, DM = device(ctx, b), device(ctx, case.a), device(ctx, case.dp), device(ctx, case.dm)
    labels = {tag: oracle.bits_from_ids(N, ids.astype(U64)) for tag, ids in case.labels.items()}
    got = {}
    for dense, fold, direct in MODES:
        with Forced(ctx, fold, direct, expand_xp_dense=dense), Folds(ctx) as ran:
            for dirty in (False, True):
                lay = ([B, A], [None, DP], [None, DM]) if dirty else ([B, A], None, None)
                key = (name, words, dense, fold, direct, dirty)
                r = engine.expand_count(ctx, src, *lay)
                print(key, r, refs[dirty]["full"])
                assert r == refs[dirty]["full"], key
                assert ctx.get_option("expand_xp_last_groups") == case.groups[dense], key
                nn, _, fl = engine.expand_count(ctx, src, *lay, want_checksum=False)
                assert (nn, fl) == (refs[dirty]["full"][0], refs[dirty]["full"][2]), key + ("count only",)
                res = [r]
                for tag, bits in labels.items():
                    rl = engine.expand_count(ctx, src, *lay, dst_label_bitmap=bits)
                    assert rl == refs[dirty][tag], key + (tag,)
                    nl, _, fl = engine.expand_count(ctx, src, *lay, dst_label_bitmap=bits, want_checksum=False)
                    assert (nl, fl) == (refs[dirty][tag][0], refs[dirty][tag][2]), key + (tag, "count only")
                    res.append(rl)
                got[(dense, fold, direct, dirty)] = tuple(res)
            assert ran.ran_only(fold) and ran.slot + ran.piece >= 12, (name, words, dense, fold, direct, ran.slot, ran.piece)
    for dirty in (False, True):
        assert len({got[(dense, fold, direct, dirty)] for dense, fold, direct in MODES}) == 1


# ---- RMAT-14 through the whole-frontier path -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat14(ctx):
    A = ctx.mat_rmat(14)
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
    ids = np.arange(0, n, dtype=U64)
    src = ids[oracle.mix64(ids) % U64(8) == 0][:1400]
    live = int(np.count_nonzero(np.diff(a.rowptr.astype(I64))[src.astype(I64)]))
    assert live > 2 * 256                                    # at least three passes of 256 live rows: one for each lane
    refs = {}
    for dirty in (False, True):
        c, flops, _ = oracle.expand_omp(src, [(a, host[0], host[1]) if dirty else (a, None, None)] * 3)
        refs[dirty] = (c.nnz, oracle.checksum_omp(c), flops)
        del c
    nd = len(np.unique(ci[: a.nnz]))
    assert 0 < nd < n
    return A, dp, dm, src, refs, {0: (n + 63) // 64, 1: (nd + 63) // 64}


def test_rmat14_whole_frontier_in_three_lanes(ctx, rmat14):
    """RMAT-14, three hops, clean and dirty, the whole-frontier path in passes of 256 live rows on 3 lanes: the oracle's tuple
    under both group forms, both folds and both direct modes, and the group count of the form that ran."""
    A, dp, dm, src, refs, groups = rmat14
    assert groups[1] < groups[0]
    got = {}
    for dense, fold, direct in MODES:
        with Forced(ctx, fold, direct, expand_xp_dense=dense, expand_scan_min=1, expand_scan_rows=256, expand_scan_lanes=3), Folds(ctx) as ran:
            for dirty in (False, True):
                lay = ([A] * 3, [dp] * 3, [dm] * 3) if dirty else ([A] * 3,)
                r = engine.expand_count(ctx, src, *lay)
                assert r == refs[dirty], (dense, fold, direct, dirty)
                assert ctx.get_option("expand_scan_last_passes") >= 3
                assert ctx.get_option("expand_xp_last_groups") == groups[dense], (dense, fold, direct, dirty)
                got[(dense, fold, direct, dirty)] = r
            assert ran.ran_only(fold), (dense, fold, direct, ran.slot, ran.piece)
    for dirty in (False, True):
        assert len({got[(dense, fold, direct, dirty)] for dense, fold, direct in MODES}) == 1


def test_dense_option_is_checked(ctx):
    before = ctx.get_option("expand_xp_dense")
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_option("expand_xp_dense", bad)
        assert ctx.get_option("expand_xp_dense") == before
    for v in (0, 1, before):
        ctx.set_option("expand_xp_dense", v)
        assert ctx.get_option("expand_xp_dense") == v
