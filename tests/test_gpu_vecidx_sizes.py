"""GPU: fgpu_vecidx_* past one workgroup of the selection, one grid of the scoring kernel and one chunk of queries, at the
largest dim, over the whole id range, and through long remove / upsert sequences — the paths of falkordb_amd/csrc/vecidx.hip
that tests/test_gpu_vecidx.py, which never stores more than 4096 vectors, leaves unrun.

Every size is derived in its test from the constants of vecidx.hip, mirrored below, and the test asserts that the size is
past its threshold with the arithmetic of fgpu_vecidx_knn's host code.  Integer stores (vc.int_store) make every f32 operation
of the euclidean and ip keys exact, so ids are compared entry for entry with the FP64 checker; cosine is compared with the
f32 key of fgpu.h rounded operation by operation (vc.keys32)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vec_check as vc  # noqa: E402
from test_gpu_vecidx import DIST_TOL, dist_close  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64

# vecidx.hip
VT = 16                     # rows per tile, components per k-chunk
SCORE_BUDGET = 256 << 20    # bytes of key images, and of survivors, per chunk of queries
SEL_PER_WG = 8192           # entries a workgroup of the selection passes reads
SEL_QUERIES_MAX = 4096
SURVIVOR_BYTES = 20         # slot, FP64 distance, u64 id
SCORE_WAVES, SCORE_WGS_PER_CU = 4, 8   # grid_for(ctx, ntiles, 4, 8): a row tile per wavefront, cus * 8 workgroups at most


def parts_of(count):
    return (count + SEL_PER_WG - 1) // SEL_PER_WG


def pad_queries(m):
    """the queries one scoring launch serves: 16, 32 or a multiple of 64"""
    return 16 if m <= 16 else 32 if m <= 32 else (m + 63) // 64 * 64


def chunk_of(count, k, nq):
    """qc of fgpu_vecidx_knn: the queries per chunk"""
    stride = (count + VT - 1) // VT * VT
    qc = min(SCORE_BUDGET // (stride * 4), SCORE_BUDGET // (min(k, count) * SURVIVOR_BYTES))
    qc = min(qc // 64 * 64, SEL_QUERIES_MAX) if qc >= 64 else 32 if qc >= 32 else 16
    return min(qc, pad_queries(nq))


def chunks_of(count, k, nq):
    """(scoring launches, query tiles) = stats[0], stats[1]"""
    qc = chunk_of(count, k, nq)
    sizes = [min(qc, nq - q0) for q0 in range(0, nq, qc)]
    return len(sizes), sum(pad_queries(m) // 16 for m in sizes)


def score_bytes(count, dim, k, nq):
    """stats[2]: every group of up to four query tiles reads the whole store once"""
    qc = chunk_of(count, k, nq)
    ntiles, nch = (count + VT - 1) // VT, (dim + VT - 1) // VT
    groups = sum(-(-(pad_queries(min(qc, nq - q0)) // 16) // 4) for q0 in range(0, nq, qc))
    return groups * ntiles * nch * 1024


@pytest.fixture
def new_index(ctx):
    """new_index(dim, metric) -> engine.VecIndex, freed when the test ends, however it ends"""
    made = []

    def new(dim, metric="euclidean"):
        made.append(engine.VecIndex(ctx, dim, metric))
        return made[-1]
    yield new
    for idx in made:
        idx.free()


def make(new_index, metric, ids, x):
    idx = new_index(x.shape[1], metric)
    idx.set(ids, x)
    assert idx.info() == (x.shape[1], engine.VEC_METRICS[metric], len(ids))
    return idx


def exact(idx, metric, ids, x, queries, k):
    """ids entry for entry the top-k by (key, id), distances within DIST_TOL, stats[3] the checker's count of ties, and the
    launch counters what the host arithmetic above says"""
    got_ids, got_d, st = idx.knn(queries, k, stats=True)
    ties = vc.check_batch(metric, ids, x, queries, k, got_ids, got_d, DIST_TOL)
    assert st[3] == ties, (st, ties)
    assert (st[0], st[1]) == chunks_of(len(ids), k, len(queries)), st
    assert st[2] == score_bytes(len(ids), x.shape[1], k, len(queries)), st
    return got_ids, got_d, st


def bits_equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(U64), b[1].view(U64))


# ---------------------------------------------------------------------------------------------------------------------------
# selection across workgroups

# (count, its parts, the k kinds): 0 -> 1, 1 -> 3, 2 -> 8192, 3 -> 8193, 4 -> count, 5 -> count + 5
PART_CASES = [(8191, 1, (0, 5)), (8192, 1, (1, 4)), (8193, 2, (0, 2, 4)), (16385, 3, (1, 3, 5)), (3 * 8192 + 5, 4, (2, 3, 4))]


def test_the_part_cases_cover_every_k_kind():
    assert {kind for _, _, kinds in PART_CASES for kind in kinds} == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("metric", ["ip", "euclidean"])
@pytest.mark.parametrize("count,parts,kinds", PART_CASES)
def test_selection_across_workgroups(ctx, new_index, metric, count, parts, kinds):
    """A query's key images are histogrammed and compacted by ceil(count / SEL_PER_WG) workgroups: counts one below, at and one
    past 8192, one past two parts, and a ragged fourth part.  At dim 2 with components in [-8, 8] a query sees at most a few
    hundred distinct keys, so every key is shared by a group of entries spread over all parts: the histogram of a digit is
    the sum of every part's, and the compaction cursor is shared by all of them."""
    assert parts_of(count) == parts and (count <= SEL_PER_WG) == (parts == 1)
    rng = np.random.default_rng(count)
    dim, nq = 2, 17
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    ids = vc.scattered_ids(rng, count)
    idx = make(new_index, metric, ids, x)
    for kind in kinds:
        k = [1, 3, 8192, 8193, count, count + 5][kind]
        _, _, st = exact(idx, metric, ids, x, queries, k)
        assert st[0] == 1
        assert (st[3] > 0) == (k < count), "below count the k-th key is shared, at count everything fits"


# ---------------------------------------------------------------------------------------------------------------------------
# the id passes of the radix select

def test_identical_vectors_under_wide_ids(ctx, new_index):
    """257 identical vectors: the four image passes decide nothing, the id passes at shift 24, 16, 8 and 0 everything, over
    ids from 0 to 2^32 - 2 that differ in the top byte alone, in the low byte alone, and anywhere between"""
    rng = np.random.default_rng(257)
    count, dim, nq = 257, 3, 3
    x = np.repeat(vc.int_store(rng, 1, dim), count, axis=0)
    ids = vc.wide_ids(rng, count)
    assert int(ids.min()) == 0 and int(ids.max()) == 2 ** 32 - 2
    queries = vc.int_store(rng, nq, dim)
    idx = make(new_index, "euclidean", ids, x)
    for k in (1, 2, 128, 256, 257):
        got_ids, _, st = exact(idx, "euclidean", ids, x, queries, k)
        assert np.array_equal(got_ids, np.tile(np.sort(ids)[:k], (nq, 1))), f"k = {k}"
        assert st[3] == (nq * count if k < count else 0)
        assert st[3] == sum(vc.expected_ties(k, vc.keys64("euclidean", q, x), ids) for q in queries)


@pytest.mark.parametrize("metric", ["ip", "euclidean"])
def test_wide_ids_across_two_parts(ctx, new_index, metric):
    """8193 vectors at dim 1 take the 17 values -8 .. 8: about 482 entries share every key, in both parts of the selection,
    and the id passes pick among them over the whole id range.  k = 300 ends inside the first group of ties, k = 600 inside
    the second."""
    count, dim, nq = SEL_PER_WG + 1, 1, 17
    assert parts_of(count) == 2
    rng = np.random.default_rng(8193)
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    assert len(np.unique(x)) == 17
    ids = vc.wide_ids(rng, count)
    idx = make(new_index, metric, ids, x)
    for k in (1, 300, 600):
        _, _, st = exact(idx, metric, ids, x, queries, k)
        assert st[3] >= nq * 300


# ---------------------------------------------------------------------------------------------------------------------------
# cosine, exactly

@pytest.mark.parametrize("count", [255, 1001])
@pytest.mark.parametrize("dim", [3, 5, 33])
def test_cosine_key_is_rounded_as_specified(ctx, new_index, dim, count):
    """fgpu.h: key = fl(1 - fl(S / fl(fl(sqrt nq) * fl(sqrt nx)))), and 1.0 when nq or nx is 0.  On integer stores S, nq and nx
    are exact, so vc.keys32 is that key and the returned SET of every query is the top-k by (keys32, id) exactly — at dim 3
    the seeds are those for which the FP64 key gives another set (tests/test_vecidx_cpu.py).  Sets, because the order inside a
    row follows the FP64 distance, not the f32 key."""
    nq = 17
    x, queries, ids = vc.cosine_case(vc.COSINE_SEEDS[dim, count], count, dim, nq)
    zero_id = set(ids[~x.any(axis=1)].tolist())
    assert len(zero_id) >= 2 and not queries[nq // 2].any()
    slot = {int(i): s for s, i in enumerate(ids)}
    idx = make(new_index, "cosine", ids, x)
    k32 = [vc.keys32("cosine", q, x) for q in queries]
    d64 = [vc.dist("cosine", q, x) for q in queries]
    for k in (1, 10, count):
        got_ids, got_d = idx.knn(queries, k)
        assert got_ids.shape == (nq, k)
        for r in range(nq):
            want = set(ids[vc.topk(k32[r], ids, k)].tolist())
            assert set(got_ids[r].tolist()) == want, f"k = {k}, query {r}"
            at = [slot[i] for i in got_ids[r].tolist()]
            assert dist_close(got_d[r], d64[r][at]), f"k = {k}, query {r}"
            dd, di = np.diff(got_d[r]), np.diff(got_ids[r].astype(np.int64))
            assert np.all((dd > 0) | ((dd == 0) & (di > 0))), f"k = {k}, query {r}: rows ascend in (D, id)"
            zeros = np.array([i in zero_id for i in got_ids[r].tolist()])
            assert np.all(got_d[r][zeros] == 1.0), f"k = {k}, query {r}"
            if k == count:
                assert zeros.sum() == len(zero_id)
        assert np.all(got_d[nq // 2] == 1.0), "the zero query is at 1.0 from everything"
        # ... and every key of the zero query is 1.0: the set is the k smallest ids
        assert sorted(got_ids[nq // 2].tolist()) == np.sort(ids)[:k].tolist()
    every_k_follows_the_f32_key(idx, ids, queries, k32)


def every_k_follows_the_f32_key(idx, ids, queries, k32):
    """the sets of k = 1 .. count together are the whole (key, id) order of the device, so a key that is off by an ulp
    anywhere in the store shows, not only one that moves an entry across the 1st or the 10th place"""
    nq, count = len(queries), len(ids)
    in_order = np.stack([ids[vc.topk(k32[r], ids, count)] for r in range(nq)])
    for k in range(1, count + 1):
        got = np.sort(idx.knn(queries, k)[0], axis=1)
        want = np.sort(in_order[:, :k], axis=1)
        assert np.array_equal(got, want), f"k = {k}, queries {np.flatnonzero((got != want).any(axis=1)).tolist()}"


@pytest.mark.parametrize("nq", [1, 17, 33])
def test_cosine_key_on_parallel_families(ctx, new_index, nq):
    """vc.parallel_case: 20 families of 50 parallel vectors, whose keys to a query differ by single ulps of the f32 key, or not
    at all, according to how sqrt, product, quotient and difference round.  For every k the returned set is the top-k by
    (keys32, id) — in the one-tile, the two-tile and the four-tile form of the scoring kernel, which must all compute the
    same key (fgpu.h: the key is a pure function of (q, x))."""
    x, queries, ids = vc.parallel_case(nq, nq)
    idx = make(new_index, "cosine", ids, x)
    k32 = [vc.keys32("cosine", q, x) for q in queries]
    assert min(len(np.unique(k)) for k in k32) > 20, "more distinct keys than families: the roundings split them"
    every_k_follows_the_f32_key(idx, ids, queries, k32)
    got_ids, got_d = idx.knn(queries, 10)
    slot = {int(i): s for s, i in enumerate(ids)}
    for r in range(nq):
        assert dist_close(got_d[r], vc.dist("cosine", queries[r], x[[slot[i] for i in got_ids[r].tolist()]])), f"query {r}"


# ---------------------------------------------------------------------------------------------------------------------------
# the scoring grid's stride loop and the chunk sizes that come from the scratch budget, on one shared store

@pytest.fixture(scope="module")
def big(ctx):
    """cus * 512 + 17 vectors at dim 3, euclidean, under wide ids; built once for the three tests below.  The scoring grid is
    capped at cus * 8 workgroups of 4 wavefronts, a row tile of 16 per wavefront: above cus * 32 tiles = cus * 512 vectors a
    wavefront takes a second tile."""
    cus = ctx.device_info()["cus"]
    assert cus >= 1
    count, dim = cus * SCORE_WGS_PER_CU * SCORE_WAVES * VT + 17, 3
    rng = np.random.default_rng(512)
    x, ids = vc.int_store(rng, count, dim), vc.wide_ids(rng, count)
    idx = engine.VecIndex(ctx, dim, "euclidean")
    try:
        idx.set(ids, x)
        assert idx.count == count
        yield SimpleNamespace(idx=idx, ids=ids, x=x, count=count, dim=dim, cus=cus)
    finally:
        idx.free()


@pytest.mark.parametrize("k", [5, 300])
def test_scoring_grid_takes_a_second_row_tile(big, k):
    """ntiles > cus * 32: the wavefronts of the first workgroups run `t += gridDim.x * 4` once more, and the last 17 vectors
    are a second tile for two of them, the last tile ragged.  The selection runs over 17 parts at 256 CUs."""
    ntiles = (big.count + VT - 1) // VT
    assert ntiles > big.cus * SCORE_WGS_PER_CU * SCORE_WAVES and parts_of(big.count) > 1
    queries = vc.int_store(np.random.default_rng(k), 17, big.dim)
    _, _, st = exact(big.idx, "euclidean", big.ids, big.x, queries, k)
    assert st[0] == 1 and st[1] == 2


def test_chunk_is_a_multiple_of_64_from_the_image_budget(big):
    """qc = floor(2^28 / (stride * 4) / 64) * 64 — 448 at 256 CUs, where stride = 131104 and 2^28 / (stride * 4) = 511.  With
    nq = qc + 2 the second chunk holds two queries: it reads `queries` from row qc, writes rows qc and qc + 1 of the result and
    runs the one-tile form of the scoring kernel after a chunk of the four-tile form."""
    k = 5
    stride = (big.count + VT - 1) // VT * VT
    qc = SCORE_BUDGET // (stride * 4) // 64 * 64
    assert 64 <= qc < SCORE_BUDGET // (k * SURVIVOR_BYTES) and qc <= SEL_QUERIES_MAX
    assert qc == 448 or big.cus != 256
    nq = qc + 2
    assert chunk_of(big.count, k, nq) == qc < pad_queries(nq)
    queries = vc.int_store(np.random.default_rng(448), nq, big.dim)
    got_ids, got_d, st = exact(big.idx, "euclidean", big.ids, big.x, queries, k)
    assert st[0] == 2 and st[1] == qc // 16 + 1
    for r in (qc - 1, qc, qc + 1):
        alone = big.idx.knn(queries[r], k)
        assert bits_equal((alone[0][0], alone[1][0]), (got_ids[r], got_d[r])), f"query {r}"


def test_chunk_of_64_from_the_survivor_budget(big):
    """k = count: the survivors (20 bytes per query and returned entry) bound the chunk, 2^28 / (count * 20) = 102 at 256 CUs,
    so qc = 64 where the key images alone would allow 448.  65 queries are two chunks, and every row is the whole store in
    (D, id) order."""
    k, nq = big.count, 65
    by_images = SCORE_BUDGET // ((big.count + VT - 1) // VT * VT * 4)
    by_survivors = SCORE_BUDGET // (k * SURVIVOR_BYTES)
    assert 64 <= by_survivors < 128 <= by_images and chunk_of(big.count, k, nq) == 64
    queries = vc.int_store(np.random.default_rng(65), nq, big.dim)
    got_ids, got_d, st = exact(big.idx, "euclidean", big.ids, big.x, queries, k)
    assert got_ids.shape == (nq, big.count)
    assert st[0] == 2 and st[1] == 4 + 1 and st[3] == 0


@pytest.mark.parametrize("count,nq,qc", [(2 ** 20 + 17, 40, 32), (2 ** 21 + 17, 20, 16)])
def test_chunks_of_32_and_of_16(ctx, new_index, count, nq, qc):
    """stride just past 2^20 (2^21): 2^28 / (stride * 4) is 63 (31), so qc takes its 32 (16) branch and the nq queries are a
    chunk of qc and a smaller one.  At dim 1 under ip a query sees at most 17 distinct keys, and the zero query one: the
    heaviest run of the id passes, over 129 (257) parts and the whole id range."""
    k = 7
    stride = (count + VT - 1) // VT * VT
    by_images = SCORE_BUDGET // (stride * 4)
    assert (32 <= by_images < 64) if qc == 32 else (by_images < 32)
    assert chunk_of(count, k, nq) == qc < nq and parts_of(count) == count // SEL_PER_WG + 1 > 128
    rng = np.random.default_rng(count)
    x, queries = vc.int_store(rng, count, 1), vc.int_store(rng, nq, 1)
    queries[3] = 0.0
    ids = vc.wide_ids(rng, count)
    idx = make(new_index, "ip", ids, x)
    _, _, st = exact(idx, "ip", ids, x, queries, k)
    assert st[0] == 2 and st[1] == qc // 16 + pad_queries(nq - qc) // 16
    assert st[3] >= count, "the zero query alone ties everything"


# ---------------------------------------------------------------------------------------------------------------------------
# query tile groups and dimension edges

@pytest.mark.parametrize("metric", ["ip", "euclidean"])
@pytest.mark.parametrize("nq,groups", [(34, 1), (64, 1), (65, 2), (129, 3)])
def test_query_tile_groups(ctx, new_index, metric, nq, groups):
    """more than 32 queries run the four-tile form; 65 and 129 are two and three groups of four query tiles (grid.y), the last
    padded, over a store of 63 row tiles of 3 k-chunks"""
    count, dim, k = 1001, 33, 10
    assert pad_queries(nq) // 16 == 4 * groups
    rng = np.random.default_rng(nq)
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    ids = vc.scattered_ids(rng, count)
    idx = make(new_index, metric, ids, x)
    _, _, st = exact(idx, metric, ids, x, queries, k)
    assert st == [1, 4 * groups, groups * 63 * 3 * 1024, st[3]]
    exact(idx, metric, ids, x, queries, count)


@pytest.mark.parametrize("metric", ["ip", "euclidean"])
@pytest.mark.parametrize("dim,nch,pad", [(4096, 256, 0), (4095, 256, 1), (4081, 256, 15), (4065, 255, 15)])
def test_dimension_edges(ctx, new_index, metric, dim, nch, pad):
    """FGPU_VECIDX_DIM_MAX and just below: 256 k-chunks with the last one full, padded by 1 and by 15, and 255 chunks, where
    the scoring loop ends in its one-chunk tail after 127 pairs.  int_store stays exact: every partial sum is within 2^18."""
    assert (dim + VT - 1) // VT == nch and nch * VT - dim == pad and dim <= 4096
    count, nq = 33, 17
    rng = np.random.default_rng(dim)
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    x[0], queries[0] = 8.0, -8.0   # the largest sums there are
    ids = vc.scattered_ids(rng, count)
    idx = make(new_index, metric, ids, x)
    for k in (7, count):
        _, _, st = exact(idx, metric, ids, x, queries, k)
        assert st[:3] == [1, 2, 3 * nch * 1024]
    for r in range(count):
        assert np.array_equal(idx.get(int(ids[r])).view(np.uint32), x[r].view(np.uint32)), f"vector {r}"


# ---------------------------------------------------------------------------------------------------------------------------
# overflowed keys under ip

@pytest.mark.parametrize("ids", [(3, 7, 5, 9), (7, 3, 5, 9)])
def test_ip_keys_that_overflow_f32_still_order(ctx, new_index, ids):
    """Query (10, 10).  (3e38, 3e38): S = +inf, key -inf, before every finite key.  (3e38, -3e38): the chain reaches +inf at
    its first step and stays there, because the key is an fmaf chain (fgpu.h): fmaf(10, -3e38, +inf) adds the exact, finite
    product -3e39 to +inf and is +inf, where a product rounded on its own would be -inf and the sum NaN.  So both keys are
    -inf, the id decides between them (either may have the smaller one), and no NaN key arises under ip at all: an infinite
    partial sum keeps its sign whatever finite product is added.  The distances are FP64: finite, and ascending in every row."""
    idx = new_index(2, "ip")
    idx.set(ids, [[3e38, 3e38], [3e38, -3e38], [1, 2], [-4, 1]])
    q = np.array([10, 10], dtype=np.float32)
    keys = np.array([-np.inf, -np.inf, -30.0, 30.0])
    for k in range(1, 5):
        got, d, st = idx.knn(q, k, stats=True)
        want = np.asarray(ids)[vc.topk(keys, ids, k)]
        assert set(got[0].tolist()) == set(want.tolist()), f"k = {k}"
        assert np.all(np.isfinite(d)) and np.all(np.diff(d[0]) >= 0), f"k = {k}"
        assert st[3] == vc.expected_ties(k, keys, ids) == (2 if k == 1 else 0)
    got, d = idx.knn(q, 4)
    assert got[0].tolist() == [ids[0], ids[2], ids[1], ids[3]]
    assert d[0].tolist() == [-(10.0 * float(np.float32(3e38))) * 2, -30.0, 0.0, 30.0]


# ---------------------------------------------------------------------------------------------------------------------------
# remove and upsert against a model

class Model:
    """id -> vector, and the slot order fgpu.h describes (a new id takes the next slot, the last vector moves into a hole):
    the order is only used to AIM the removals, every assertion is on the dict"""

    def __init__(self):
        self.vec, self.slots, self.gone = {}, [], set()

    def set(self, ids, vecs):
        for i, v in zip(ids, vecs):
            if i not in self.vec:
                self.slots.append(i)
                self.gone.discard(i)
            self.vec[i] = v

    def remove(self, ids):
        n = 0
        for i in ids:
            if i in self.vec:
                s = self.slots.index(i)
                self.slots[s] = self.slots[-1]
                self.slots.pop()
                del self.vec[i]
                self.gone.add(i)
                n += 1
        return n


def aimed_removals(rng, model, want):
    """about `want` present ids, in an order that makes the move planning work: an id and then the id that moves into its
    hole; the id of the last slot, then ids before it — and among them absent ids, repeats and ids that do not fit"""
    sim, batch = list(model.slots), []

    def take(i):
        s = sim.index(i)
        sim[s] = sim[-1]
        sim.pop()
        batch.append(i)
    if want >= 2 and len(sim) >= 3:        # an id before the last slot; the last vector moves into its hole, and goes next
        take(sim[int(rng.integers(0, len(sim) - 1))])
        take(model.slots[-1])
    if want - len(batch) >= 3 and len(sim) >= 4:   # the last slot together with ids before it, in either order
        last, before = sim[-1], [sim[int(j)] for j in rng.choice(len(sim) - 1, size=2, replace=False)]
        for i in ([last] + before) if rng.random() < 0.5 else (before + [last]):
            take(i)
    while sim and len(batch) < want:
        take(sim[int(rng.integers(0, len(sim)))])
    present = len(batch)
    extra = [int(rng.integers(2 ** 33, 2 ** 34)), 2 ** 32 - 1 if rng.random() < 0.5 else 2 ** 63]   # never stored, never fit
    extra += [int(i) for i in rng.permutation(sorted(model.gone))[:2]]
    extra += [batch[int(j)] for j in rng.integers(0, len(batch), size=2)] if batch else []
    for i in extra:
        batch.insert(int(rng.integers(0, len(batch) + 1)), i)
    return batch, present


def test_remove_and_upsert_against_a_model(ctx, new_index):
    """A fixed-seed sequence of set and remove batches, the count moving between 0 and about 700: across 16-slot tile edges and
    the capacity doublings at 256 and 512.  After every call the return value and the count are the model's; at tile-aligned
    counts and every tenth step every live vector comes back bit for bit, removed ids are absent, and a search for
    count + 5 neighbours is exact, so nothing stale past `count` surfaces."""
    rng = np.random.default_rng(700)
    dim = 5
    idx, model = new_index(dim, "euclidean"), Model()
    queries = vc.int_store(rng, 3, dim)
    pool = [int(i) for i in vc.wide_ids(rng, 4000)]   # new ids come from here, in this order
    steps = full = 0
    seen_counts = []

    def full_check():
        live = np.array(model.slots, dtype=U64)
        assert sorted(model.slots) == sorted(model.vec)
        for i in model.slots:
            assert np.array_equal(idx.get(i).view(np.uint32), model.vec[i].view(np.uint32)), f"id {i} at step {steps}"
        for i in model.gone:
            assert idx.get(i) is None, f"id {i} at step {steps}"
        assert idx.get(2 ** 32 - 1) is None and idx.get(2 ** 63) is None
        if len(live):
            x = np.stack([model.vec[i] for i in model.slots])
            exact(idx, "euclidean", live, x, queries, len(live) + 5)
        else:
            assert idx.knn(queries, 5)[0].shape == (3, 0)

    for target in (300, 240, 530, 500, 700, 0, 60, 17, 16, 0, 33, 272, 256):
        while len(model.vec) != target:
            n = len(model.vec)
            if n < target:
                m = min(int(rng.integers(1, 24)), target - n)
                back = [int(rng.permutation(sorted(model.gone))[0])] if model.gone and m >= 2 and rng.random() < 0.5 else []
                fresh = [pool.pop() for _ in range(m - len(back))] + back     # (an id that was removed comes back)
                old = [model.slots[int(j)] for j in rng.integers(0, n, size=min(n, 4))] if n else []
                batch = fresh + old + [fresh[0], fresh[-1]] + old[:1]         # repeats: the last row of an id wins
                batch = [batch[int(j)] for j in rng.permutation(len(batch))]
                vecs = vc.int_store(rng, len(batch), dim)
                idx.set(np.array(batch, dtype=U64), vecs)
                model.set(batch, vecs)
            else:
                batch, present = aimed_removals(rng, model, min(int(rng.integers(6, 24)), n - target))
                assert model.remove(batch) == present >= 1
                assert idx.remove(np.array(batch, dtype=U64)) == present, f"step {steps}"
            steps += 1
            count = len(model.vec)
            seen_counts.append(count)
            assert idx.count == count, f"step {steps}"
            if count % VT == 0 or steps % 10 == 0:
                full_check()
                full += 1
    full_check()
    assert 150 <= steps <= 300 and full >= 20, (steps, full)
    assert max(seen_counts) >= 700 and 0 in seen_counts and any(c > 512 for c in seen_counts)
