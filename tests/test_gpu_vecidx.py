"""GPU: fgpu_vecidx_* (the exhaustive vector search behind db.idx.vector.queryNodes / queryRelationships) against the FP64
checker of tests/vec_check.py.  Integer inputs make every f32 operation of the key exact, so ids are compared entry for
entry; float inputs are held to the band rule with the f32 rounding bound of the key; a query alone and inside a batch must
agree bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vec_check as vc  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
DIST_TOL = 1e-12   # the FP64 accumulation bound dim * 2^-53 at FGPU_VECIDX_DIM_MAX, rounded up


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
    assert idx.info() == (x.shape[1], engine.VEC_METRICS[metric], len(set(np.asarray(ids).tolist())))
    return idx


def dist_close(got, want):
    return np.all(np.abs(got - want) <= DIST_TOL * np.maximum(1.0, np.abs(want)))


def check_exact(idx, metric, ids, x, queries, k):
    """ids entry for entry the checker's top-k by (key, id), dist within the FP64 accumulation bound"""
    got_ids, got_d, st = idx.knn(queries, k, stats=True)
    kk = min(k, len(ids))
    assert got_ids.shape == (len(queries), kk) and got_d.shape == (len(queries), kk)
    for r, q in enumerate(queries):
        top = vc.topk(vc.keys64(metric, q, x), ids, k)
        assert got_ids[r].tolist() == ids[top].tolist(), f"query {r}"
        assert dist_close(got_d[r], vc.dist(metric, q, x[top])), f"query {r}"
    return st


DIMS = [1, 2, 3, 4, 5, 33, 64, 130]
COUNTS = [1, 15, 16, 17, 255, 257, 1001]
NQS = [1, 16, 17, 33]
# (dim, count, nq, k kind, metric): every listed dim, count, nq and k kind appears at least once
INT_CASES = [(d, COUNTS[i % 7], NQS[i % 4], i % 4, ("euclidean", "ip")[i % 2]) for i, d in enumerate(DIMS)] + [
    (130, 1001, 33, 1, "ip"), (64, 257, 17, 3, "euclidean"), (5, 1001, 16, 2, "euclidean"), (33, 17, 1, 0, "ip"),
    (3, 255, 33, 1, "ip"), (4, 16, 17, 2, "euclidean")]


def test_the_sampled_product_covers_every_listed_value():
    assert {c[0] for c in INT_CASES} == set(DIMS) and {c[1] for c in INT_CASES} == set(COUNTS)
    assert {c[2] for c in INT_CASES} == set(NQS) and {c[3] for c in INT_CASES} == {0, 1, 2, 3}
    assert {c[4] for c in INT_CASES} == {"euclidean", "ip"}


@pytest.mark.parametrize("dim,count,nq,kkind,metric", INT_CASES)
def test_integer_inputs_exact(ctx, new_index, dim, count, nq, kkind, metric):
    rng = np.random.default_rng(1000 * dim + count + nq)
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    ids = vc.scattered_ids(rng, count)
    k = [1, 3, count, count + 5][kkind]
    idx = make(new_index, metric, ids, x)
    st = check_exact(idx, metric, ids, x, queries, k)
    assert st[0] >= 1 and st[1] >= (nq + 15) // 16
    assert st[2] >= st[0] * ((count + 15) // 16) * ((dim + 15) // 16) * 1024


@pytest.mark.parametrize("metric", ["euclidean", "ip"])
def test_identical_vectors_are_decided_by_id(ctx, new_index, metric):
    rng = np.random.default_rng(5)
    count, dim, nq, k = 257, 33, 17, 40
    x = np.repeat(vc.int_store(rng, 1, dim), count, axis=0)
    ids = vc.scattered_ids(rng, count)
    queries = vc.int_store(rng, nq, dim)
    idx = make(new_index, metric, ids, x)
    st = check_exact(idx, metric, ids, x, queries, k)
    got_ids, _ = idx.knn(queries, k)
    assert np.array_equal(got_ids, np.tile(np.sort(ids)[:k], (nq, 1)))
    assert st[3] == nq * count          # every entry tied the k-th key, in every query
    assert st[3] == sum(vc.expected_ties(k, vc.keys64(metric, q, x), ids) for q in queries)
    st_all = check_exact(idx, metric, ids, x, queries, count)
    assert st_all[3] == 0               # ... and when all of them fit there is nothing to decide
    assert st_all[3] == sum(vc.expected_ties(count, vc.keys64(metric, q, x), ids) for q in queries)


def test_ties_are_counted(ctx, new_index):
    # components in {0, 1} at dim 2: four distinct euclidean keys at most, so the k-th key is shared
    rng = np.random.default_rng(11)
    x = rng.integers(0, 2, size=(255, 2)).astype(np.float32)
    ids = vc.scattered_ids(rng, 255)
    idx = make(new_index, "euclidean", ids, x)
    st = check_exact(idx, "euclidean", ids, x, np.zeros((1, 2), dtype=np.float32), 3)
    assert st[3] > 0
    assert st[3] == vc.expected_ties(3, vc.keys64("euclidean", np.zeros(2, dtype=np.float32), x), ids)


@pytest.mark.parametrize("dim,places", [(4, (0, 1, 2, 3)), (16, (1, 6, 11, 12)), (33, (0, 5, 18, 32)), (33, (15, 16, 31, 32))])
def test_key_is_the_index_ordered_f32_chain(ctx, new_index, dim, places):
    """fgpu.h: S(q, x) is the fmaf chain from 0 over i = 0 .. dim - 1.  2^24, 1, -2^24 and 1 in every order, at places inside
    one MFMA, across its four steps and across k-chunks, against a query of ones: every product is exact, so the chain is a
    chain of f32 additions whose result (0, 1 or 2) depends on the order alone — and FP64 gives 2 for all of them, so the
    selection is the only place the f32 key shows."""
    import itertools
    vals = (2.0 ** 24, 1.0, -2.0 ** 24, 1.0)
    perms = sorted(set(itertools.permutations(vals)))
    x = np.zeros((len(perms), dim), dtype=np.float32)
    for r, p in enumerate(perms):
        x[r, list(places)] = p
    q = np.ones(dim, dtype=np.float32)
    keys = vc.keys32("ip", q, x)
    assert set(keys.tolist()) == {0.0, -1.0, -2.0}
    ids = vc.scattered_ids(np.random.default_rng(dim), len(perms))
    idx = make(new_index, "ip", ids, x)
    for k in range(1, len(perms) + 1):
        got_ids, got_d = idx.knn(q, k)
        assert sorted(got_ids[0].tolist()) == sorted(ids[vc.topk(keys, ids, k)].tolist()), f"k = {k}"
        assert np.all(got_d == -2.0) and np.all(np.diff(got_ids[0].astype(np.int64)) > 0)


@pytest.mark.parametrize("metric", ["euclidean", "ip"])
def test_queries_in_several_chunks(ctx, new_index, metric):
    """4100 queries are more than one chunk holds (4096): the second chunk reads its own queries, writes its own rows of the
    result and runs the one-tile form of the scoring kernel; the counters add up over both"""
    rng = np.random.default_rng(41)
    count, dim, nq, k = 16, 3, 4100, 3
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    ids = vc.scattered_ids(rng, count)
    idx = make(new_index, metric, ids, x)
    st = check_exact(idx, metric, ids, x, queries, k)
    assert st[0] == 2 and st[1] == 4096 // 16 + 1 and st[2] == (4096 // 64 + 1) * 1024
    single = idx.knn(queries[4097], k)
    batch = idx.knn(queries, k)
    assert np.array_equal(single[0][0], batch[0][4097]) and np.array_equal(single[1][0].view(U64), batch[1][4097].view(U64))
    check_exact(idx, metric, ids, x, queries[:4100], count + 5)   # every entry of every row, ties by id throughout


def test_keys_that_overflow_f32_still_order(ctx, new_index):
    """fgpu.h: finite components can overflow the f32 key; +inf orders above every finite key and a NaN key after +inf.  Against
    q = (1e20, 0): the vector (1e20, 0) has the key inf - inf, the small ones inf - finite, so the selection by key takes the small
    ones first, in id order, although FP64 knows better; the reported distances are FP64 and exact."""
    idx = new_index(2, "euclidean")
    idx.set([1, 5, 4, 9], [[1e20, 0], [1, 0], [2, 0], [1e20, 1]])
    q = np.array([1e20, 0], dtype=np.float32)
    for k, want in ((1, {4}), (2, {4, 5}), (3, {1, 4, 5}), (4, {1, 4, 5, 9})):
        ids, d = idx.knn(q, k)
        assert set(ids[0].tolist()) == want, f"k = {k}"
        assert np.all(np.isfinite(d)) and np.all(np.diff(d[0]) >= 0)
    ids, d = idx.knn(q, 4)
    assert ids[0].tolist() == [1, 9, 4, 5] and d[0, 0] == 0.0 and d[0, 1] == 1.0


@pytest.mark.parametrize("metric", vc.METRICS)
def test_batch_and_single_agree_bitwise(ctx, new_index, metric):
    x, queries = vc.float_store(1000, 33, 33)
    ids = vc.scattered_ids(np.random.default_rng(2), 1000)
    idx = make(new_index, metric, ids, x)
    b_ids, b_d = idx.knn(queries, 7)
    for r in range(33):
        s_ids, s_d = idx.knn(queries[r], 7)
        assert np.array_equal(s_ids[0], b_ids[r]), f"query {r}"
        assert np.array_equal(s_d[0].view(U64), b_d[r].view(U64)), f"query {r}"


@pytest.mark.parametrize("metric", vc.METRICS)
@pytest.mark.parametrize("count,dim,nq,k", [(4096, 64, 64, 10), (1000, 33, 17, 7)])
def test_float_inputs_band_rule(ctx, new_index, metric, count, dim, nq, k):
    x, queries = vc.float_store(count, dim, nq)
    ids = np.arange(count, dtype=U64)
    idx = make(new_index, metric, ids, x)
    got_ids, got_d = idx.knn(queries, k)
    busy = 0
    for r, q in enumerate(queries):
        keys = vc.keys64(metric, q, x)
        m = vc.margin(metric, q, x)
        _, b = vc.band(k, keys, ids, m)
        busy += len(b) > 1
        assert vc.band_ok(got_ids[r], k, keys, m), f"query {r}"
        assert dist_close(got_d[r], vc.dist(metric, q, x[got_ids[r].astype(np.int64)])), f"query {r}"
        assert np.all(np.diff(got_d[r]) >= 0), f"query {r}"
    assert busy * 8 <= nq, "the inputs must leave the band empty for all but 1 query in 8"


def test_upsert_replaces(ctx, new_index):
    # test_vecsim.py test08: set, set the same value again, set another value; k = 1 finds the node at its new place
    idx = new_index(2, "euclidean")
    idx.set([1, 2, 3], [[0, 0], [5, 5], [9, 9]])
    idx.set([2], [[5, 5]])
    assert idx.count == 3 and idx.knn([5, 5], 1)[0].tolist() == [[2]]
    idx.set([2], [[20, 20]])
    assert idx.count == 3
    ids, d = idx.knn([5, 5], 1)
    assert ids.tolist() == [[3]] and d[0, 0] == np.sqrt(32.0)
    ids, d = idx.knn([20, 20], 1)
    assert ids.tolist() == [[2]] and d[0, 0] == 0.0
    assert idx.get(2).tolist() == [20.0, 20.0]


def test_duplicate_id_in_one_call_last_wins(ctx, new_index):
    idx = new_index(3, "euclidean")
    idx.set([7, 8, 7, 9, 7], [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 5]])
    assert idx.count == 3 and idx.get(7).tolist() == [5.0, 5.0, 5.0]
    idx.set([8, 8], [[6, 6, 6], [0, 0, 0]])
    assert idx.count == 3 and idx.get(8).tolist() == [0.0, 0.0, 0.0]
    ids, d = idx.knn([5, 5, 5], 3)
    assert ids.tolist() == [[7, 9, 8]]


def test_remove_last_first_middle(ctx, new_index):
    rng = np.random.default_rng(21)
    count, dim = 100, 5
    x = vc.int_store(rng, count, dim)
    ids = vc.scattered_ids(rng, count)
    idx = make(new_index, "euclidean", ids, x)
    queries = vc.int_store(rng, 3, dim)
    keep = np.ones(count, dtype=bool)
    for slot in (count - 1, 0, 50):
        assert idx.remove([ids[slot]]) == 1
        keep[slot] = False
        assert idx.count == keep.sum() and idx.get(int(ids[slot])) is None
        check_exact(idx, "euclidean", ids[keep], x[keep], queries, 10)
        check_exact(idx, "euclidean", ids[keep], x[keep], queries, count)
    # several at once, absent and repeated ids among them
    gone = [int(ids[3]), int(ids[97]), int(ids[98]), 10 ** 9, int(ids[3]), int(ids[slot])]
    assert idx.remove(gone) == 3
    keep[[3, 97, 98]] = False
    check_exact(idx, "euclidean", ids[keep], x[keep], queries, count)
    for r in np.nonzero(keep)[0]:
        assert np.array_equal(idx.get(int(ids[r])), x[r])


def test_growth_across_a_capacity_doubling_keeps_every_vector(ctx, new_index):
    rng = np.random.default_rng(22)
    dim = 7
    x = rng.uniform(-1, 1, (700, dim)).astype(np.float32)
    ids = vc.scattered_ids(rng, 700)
    idx = new_index(dim, "cosine")
    for lo, hi in ((0, 200), (200, 300), (300, 700)):   # the store starts at 256 slots: both later calls outgrow it
        idx.set(ids[lo:hi], x[lo:hi])
        assert idx.count == hi
        for r in range(hi):
            assert np.array_equal(idx.get(int(ids[r])), x[r]), f"vector {r} after {hi}"


def test_remove_everything(ctx, new_index):
    idx = new_index(4, "ip")
    idx.set(np.arange(40), np.ones((40, 4), dtype=np.float32))
    assert idx.remove(np.arange(40)) == 40 and idx.count == 0
    ids, d = idx.knn(np.ones(4), 5)
    assert ids.shape == (1, 0) and d.shape == (1, 0)
    idx.set([3], [[1, 2, 3, 4]])
    assert idx.knn([1, 0, 0, 0], 5)[0].tolist() == [[3]]


def code_of(call):
    with pytest.raises(FgpuError) as e:
        call()
    assert str(e.value).split(":", 1)[1].strip(), "fgpu_last_error is set"
    return e.value.code


def test_errors(ctx, new_index):
    lib = ctx.lib
    fp = C.POINTER(C.c_float)
    h = C.c_void_p()
    for dim in (0, 4097):
        assert code_of(lambda: new_index(dim, "euclidean")) == _ffi.FGPU_INVALID
    assert code_of(lambda: new_index(4, 7)) == _ffi.FGPU_INVALID
    assert lib.fgpu_vecidx_new(ctx._h, None, 4, 0) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_new(None, C.byref(h), 4, 0) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_last_error()
    idx = new_index(4, "euclidean")   # FGPU_VECIDX_DIM_MAX itself is fine
    new_index(4096, "ip")
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    idx.set([10, 11, 12], x)
    one = np.ones(4, dtype=np.float32)
    got, kk = np.zeros(3, dtype=U64), C.c_uint64(99)
    d = np.zeros(3, dtype=np.float64)
    dp, ip = d.ctypes.data_as(C.POINTER(C.c_double)), got.ctypes.data_as(_ffi.u64p)
    assert code_of(lambda: idx.set([2 ** 32 - 1], [one])) == _ffi.FGPU_INVALID
    assert code_of(lambda: idx.set([2 ** 40], [one])) == _ffi.FGPU_INVALID
    idx.set([2 ** 32 - 2], [one])
    assert idx.remove([2 ** 32 - 2, 2 ** 32 - 1, 2 ** 63]) == 1
    assert code_of(lambda: idx.knn(one, 0)) == _ffi.FGPU_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        q = one.copy()
        q[2] = bad
        assert code_of(lambda: idx.knn(q, 1)) == _ffi.FGPU_INVALID
        # a rejected set leaves the store as it was, the valid rows of the call included
        assert code_of(lambda: idx.set([10, 13], np.stack([one, q]))) == _ffi.FGPU_INVALID
        assert idx.count == 3 and idx.get(13) is None and np.array_equal(idx.get(10), x[0])
    assert lib.fgpu_vecidx_set(ctx._h, idx._h, None, one.ctypes.data_as(fp), 1) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_set(ctx._h, None, ip, one.ctypes.data_as(fp), 1) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_remove(ctx._h, idx._h, None, 1, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_get(ctx._h, idx._h, 10, None, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_info(None, None, None, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_knn(ctx._h, idx._h, one.ctypes.data_as(fp), 1, 1, ip, dp, None, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_knn(ctx._h, idx._h, None, 1, 1, ip, dp, C.byref(kk), None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_knn(ctx._h, idx._h, one.ctypes.data_as(fp), 1, 1, None, dp, C.byref(kk), None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_vecidx_knn(None, idx._h, one.ctypes.data_as(fp), 1, 1, ip, dp, C.byref(kk), None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_last_error()
    # nq == 0 does nothing, whatever the arrays
    assert lib.fgpu_vecidx_knn(ctx._h, idx._h, None, 0, 5, None, None, C.byref(kk), None) == _ffi.FGPU_OK and kk.value == 0
    # after all of it the index still works
    check_exact(idx, "euclidean", np.array([10, 11, 12], dtype=U64), x, np.stack([one, x[2]]), 2)
    assert lib.fgpu_vecidx_free(None) == _ffi.FGPU_OK
