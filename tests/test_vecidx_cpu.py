"""CPU: the checker of the vector index tests (tests/vec_check.py) on hand-worked cases, the band rule on a constructed
near-tie, and the exactness claim the integer GPU tests rest on: for their generators the f32 key, rounded operation by
operation, equals the FP64 key, so the (key, id) order the device must return is known exactly."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vec_check as vc  # noqa: E402


def test_hand_worked_distances():
    # test_vecsim.py test01: [1, 2] against [2, 3]
    assert round(float(vc.dist("euclidean", [1, 2], [2, 3])[0]), 3) == 1.414
    assert round(float(vc.dist("cosine", [1, 2], [2, 3])[0]), 3) == 0.008
    assert vc.dist("euclidean", [1, 2], [2, 3])[0] == math.sqrt(2.0)
    assert vc.dist("ip", [1, 2], [2, 3])[0] == -8.0
    x = np.array([[0.25, -3.0, 7.5]], dtype=np.float32)
    assert vc.dist("euclidean", x[0], x)[0] == 0.0
    assert abs(vc.dist("cosine", x[0], x)[0]) <= 2.0 ** -50
    assert vc.dist("ip", x[0], x)[0] == -float(np.sum(x.astype(np.float64) ** 2))


def test_zero_vector_under_cosine_is_one():
    z = np.zeros(3, dtype=np.float32)
    x = np.array([[1, 2, 3], [0, 0, 0]], dtype=np.float32)
    assert vc.dist("cosine", z, x).tolist() == [1.0, 1.0]
    assert vc.dist("cosine", x[0], x).tolist()[1] == 1.0
    assert vc.keys64("cosine", z, x).tolist() == [1.0, 1.0]


def test_rows_are_scored_one_by_one():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (17, 5)).astype(np.float32)
    q = rng.uniform(-1, 1, 5).astype(np.float32)
    for metric in vc.METRICS:
        whole = vc.dist(metric, q, x)
        assert whole.shape == (17,)
        for r in range(17):
            assert vc.dist(metric, q, x[r])[0] == whole[r]
    # the euclidean key is the squared distance
    assert np.allclose(vc.keys64("euclidean", q, x), vc.dist("euclidean", q, x) ** 2, rtol=1e-12, atol=1e-12)


def test_topk_orders_by_key_then_id():
    keys = np.array([2.0, 1.0, 1.0, 3.0, 1.0])
    ids = np.array([10, 40, 20, 5, 30])
    assert ids[vc.topk(keys, ids, 3)].tolist() == [20, 30, 40]
    assert ids[vc.topk(keys, ids, 4)].tolist() == [20, 30, 40, 10]
    assert len(vc.topk(keys, ids, 99)) == 5


def test_band_rule_on_a_constructed_near_tie():
    # keys: two clear winners, then two entries 1e-9 apart around the 3rd place, then a clear loser
    keys = np.array([0.1, 0.2, 0.5, 0.5 + 1e-9, 0.9])
    m = 1e-8
    top, b = vc.band(3, keys, np.arange(5), m)
    assert top == {0, 1, 2} and b == {2, 3}
    assert vc.band_ok([0, 1, 2], 3, keys, m)
    assert vc.band_ok([1, 0, 3], 3, keys, m)          # the near-tie may fall either way
    assert not vc.band_ok([0, 1, 4], 3, keys, m)      # a clear loser may not enter
    assert not vc.band_ok([0, 2, 3], 3, keys, m)      # a clear winner may not leave
    assert not vc.band_ok([0, 1], 3, keys, m)
    assert not vc.band_ok([0, 1, 3], 3, keys, 1e-10)  # with a tight bound the order is decided
    # ids other than the positions
    assert vc.band_ok([70, 50, 90], 3, keys, m, ids=np.array([50, 70, 80, 90, 60]))


def test_margins():
    x, q = vc.float_store(100, 33, 2)
    g = vc.gamma(36)
    assert g == 36 * 2.0 ** -24 / (1 - 36 * 2.0 ** -24)
    assert vc.margin("cosine", q[0], x) == 3 * vc.gamma(37)
    ab = np.abs(x.astype(np.float64)) @ np.abs(q[0].astype(np.float64))
    assert math.isclose(vc.margin("ip", q[0], x), vc.gamma(34) * ab.max(), rel_tol=1e-12)
    sq = (x.astype(np.float64) ** 2).sum(1) + float((q[0].astype(np.float64) ** 2).sum())
    assert math.isclose(vc.margin("euclidean", q[0], x), g * (sq + 2 * ab).max(), rel_tol=1e-12)


@pytest.mark.parametrize("metric", ["euclidean", "ip"])
@pytest.mark.parametrize("dim", [1, 2, 3, 4, 5, 33, 64, 130])
def test_integer_generators_make_the_f32_key_exact(metric, dim):
    rng = np.random.default_rng(100 + dim)
    x = vc.int_store(rng, 257, dim)
    q = vc.int_store(rng, 4, dim)
    assert np.abs(x).max() <= 8 and np.all(x == np.round(x))
    for r in range(4):
        k32 = vc.keys32(metric, q[r], x)
        k64 = vc.keys64(metric, q[r], x)
        assert k32.dtype == np.float32
        assert np.array_equal(k32.astype(np.float64), k64)
        assert np.abs(k64).max() < 2 ** 24


@pytest.mark.parametrize("metric", ["euclidean", "ip"])
@pytest.mark.parametrize("dim", [4065, 4081, 4095, 4096])
def test_integer_generators_stay_exact_up_to_dim_max(metric, dim):
    """the dims of tests/test_gpu_vecidx_sizes.py, with the extreme rows beside the random ones: all components 8 against
    queries of all 8 and all -8 reach the bounds of int_store's docstring, 2^18 for a chain and 2^20 for the euclidean key"""
    rng = np.random.default_rng(100 + dim)
    x = np.concatenate([vc.int_store(rng, 31, dim), np.full((1, dim), 8, np.float32), np.full((1, dim), -8, np.float32)])
    q = np.concatenate([vc.int_store(rng, 2, dim), np.full((1, dim), 8, np.float32), np.full((1, dim), -8, np.float32)])
    for r in range(4):
        k32 = vc.keys32(metric, q[r], x)
        k64 = vc.keys64(metric, q[r], x)
        assert k32.dtype == np.float32 and np.array_equal(k32.astype(np.float64), k64)
        assert np.abs(k64).max() <= 2 ** 20 < 2 ** 24
    assert np.abs(vc.keys64("ip", q[2], x)).max() == 64 * dim and vc.keys64("euclidean", q[2], x).max() == 256 * dim
    assert np.array_equal(vc.batch_keys(metric, q, x), np.stack([vc.keys64(metric, q[r], x) for r in range(4)]))


def test_cosine_key32_hand_worked():
    """axis vectors scaled by powers of two: every sqrt, product and quotient is exact, the keys are 0, 1 and 2"""
    x = np.array([[4, 0, 0], [0, 0.5, 0], [-8, 0, 0], [0.25, 0, 0], [0, 0, -2]], dtype=np.float32)
    k = vc.keys32("cosine", [16, 0, 0], x)
    assert k.dtype == np.float32 and k.tolist() == [0.0, 1.0, 2.0, 0.0, 1.0]
    assert vc.keys32("cosine", [0, -0.125, 0], x).tolist() == [1.0, 2.0, 1.0, 1.0, 1.0]
    assert np.array_equal(k.astype(np.float64), vc.keys64("cosine", [16, 0, 0], x))
    # every step rounded on its own: (1, 1) against (1, 0) is fl(1 - fl(1 / fl(sqrt 2)))
    r2 = np.sqrt(np.float32(2.0))
    assert vc.keys32("cosine", [1, 1], [[1, 0]])[0] == np.float32(1.0) - np.float32(1.0) / r2
    # the denominator is the PRODUCT OF THE ROUNDED ROOTS, not the root of the product: (1, 1) with itself
    assert vc.keys32("cosine", [1, 1], [[1, 1]])[0] == np.float32(1.0) - np.float32(2.0) / (r2 * r2)
    assert r2 * r2 != np.float32(2.0) and vc.keys32("cosine", [1, 1], [[1, 1]])[0] != 0.0


def test_cosine_key32_zero_rule():
    z = np.zeros(3, dtype=np.float32)
    x = np.array([[1, 2, 3], [0, 0, 0], [-0.0, 0, 0]], dtype=np.float32)
    assert vc.keys32("cosine", z, x).tolist() == [1.0, 1.0, 1.0]
    assert vc.keys32("cosine", x[0], x).tolist()[1:] == [1.0, 1.0]
    assert vc.keys32("cosine", x[0], x).dtype == np.float32


@pytest.mark.parametrize("count", [255, 1001])
def test_cosine_f32_and_fp64_top_k_differ_at_dim_3(count):
    """the pinned cases the exact cosine GPU test rests on: with these seeds some query's top-10 by the f32 key is another set
    than by the FP64 key, so a device key that is not rounded step by step as fgpu.h says is told apart"""
    x, q, ids = vc.cosine_case(vc.COSINE_SEEDS[3, count], count, 3, 17)
    assert not x[count // 2].any() and not q[8].any() and 2 <= (~x.any(axis=1)).sum() <= count // 10
    differ = 0
    for r in range(17):
        k32, k64 = vc.keys32("cosine", q[r], x), vc.keys64("cosine", q[r], x)
        assert np.abs(k32 - k64).max() <= vc.margin("cosine", q[r], x)
        differ += set(vc.topk(k32, ids, 10).tolist()) != set(vc.topk(k64, ids, 10).tolist())
    assert differ >= 1


def test_parallel_families_split_by_single_roundings():
    """what test_cosine_key_on_parallel_families rests on: the chains are exact, a query's f32 keys to its own family take
    several values an ulp of 1.0 apart where FP64 sees them within 2^-50 of each other, and a key with the root of the product
    in place of the product of the roots orders the store otherwise"""
    x, q, ids = vc.parallel_case(17, 17)
    assert x.shape == (1001, 3) and np.abs(x).max() <= 1800 and np.all(x == np.round(x))
    assert (x.astype(np.float64) ** 2).sum(1).max() < 2 ** 24
    f = np.float32
    moved = 0
    for r in range(17):
        k32, k64 = vc.keys32("cosine", q[r], x), vc.keys64("cosine", q[r], x)
        own = np.abs(k64) < 2.0 ** -40
        assert own.sum() >= 50 and np.abs(k64[own]).max() <= 2.0 ** -50
        assert len(np.unique(k32[own])) >= 2 and np.abs(k32[own]).max() <= 4 * 2.0 ** -24
        nq, nx, s = (q[r] * q[r]).sum(dtype=f), (x * x).sum(1, dtype=f), (x * q[r]).sum(1, dtype=f)
        other = f(1.0) - s / np.sqrt(nq * nx)
        assert other.dtype == f
        moved += vc.topk(other, ids, 1001).tolist() != vc.topk(k32, ids, 1001).tolist()
    assert moved >= 10


def test_expected_ties():
    # every vector identical: all tie; the id order decides unless all of them fit
    same = np.full(40, 2.5)
    ids = vc.scattered_ids(np.random.default_rng(4), 40)
    for k in (1, 7, 39):
        assert vc.expected_ties(k, same, ids) == 40
    assert vc.expected_ties(40, same, ids) == 0 and vc.expected_ties(45, same, ids) == 0
    # no tie at the k-th key
    keys = np.array([3.0, 1.0, 2.0, 2.0, 5.0, 4.0])
    assert vc.expected_ties(1, keys) == 0 and vc.expected_ties(4, keys) == 0 and vc.expected_ties(5, keys) == 0
    # a tie that fits exactly is not counted, one that does not fit is counted whole
    assert vc.expected_ties(3, keys) == 0 and vc.expected_ties(2, keys) == 2
    assert vc.expected_ties(2, np.array([1.0, 0.0, -0.0, 0.0])) == 3   # -0.0 = +0.0
    assert vc.expected_ties(3, np.array([], dtype=np.float64)) == 0


def test_wide_ids():
    for count in (8, 257, 8193):
        ids = vc.wide_ids(np.random.default_rng(count), count)
        assert ids.dtype == np.uint64 and len(ids) == count and len(set(ids.tolist())) == count
        assert int(ids.min()) == 0 and int(ids.max()) == 2 ** 32 - 2 == vc.ID_MAX
        have = set(ids.tolist())
        top = sum(1 for a in have for s in range(1, 256) if (a ^ (s << 24)) in have) // 2
        low = sum(1 for a in have for s in range(1, 256) if (a ^ s) in have) // 2
        assert top >= max(3, (count - 8) // 3) and low >= max(3, (count - 8) // 3), (top, low)
        assert {1 << 24, 0xFF, vc.ID_MAX ^ (0xFF << 24), vc.ID_MAX ^ 0xFE} <= have
        assert np.any(np.diff(ids.astype(np.int64)) < 0), "not in order"
        if count > 8:   # every byte takes many values: the four id passes each see more than digit 0
            for shift in (0, 8, 16, 24):
                assert len({(i >> shift) & 255 for i in have}) > min(100, count // 4)
    assert np.array_equal(vc.wide_ids(np.random.default_rng(3), 100), vc.wide_ids(np.random.default_rng(3), 100))


@pytest.mark.parametrize("metric", ["euclidean", "ip"])
def test_batch_check_agrees_with_the_per_query_checker(metric):
    """dim 2 in [-8, 8] at count 300: keys tie in groups, at the k-th place too"""
    rng = np.random.default_rng(9)
    count, dim, nq = 300, 2, 23
    x, queries = vc.int_store(rng, count, dim), vc.int_store(rng, nq, dim)
    ids = vc.wide_ids(rng, count)
    keys = vc.batch_keys(metric, queries, x)
    assert keys.shape == (nq, count)
    for r in range(nq):
        assert np.array_equal(keys[r], vc.keys64(metric, queries[r], x))
    for k in (1, 3, 50, 299, 300, 305):
        top, ties = vc.batch_topk(keys, ids, k)
        assert top.shape == (nq, min(k, count))
        for r in range(nq):
            assert top[r].tolist() == vc.topk(keys[r], ids, k).tolist(), (k, r)
        assert ties == sum(vc.expected_ties(k, keys[r], ids) for r in range(nq))
        assert ties > 0 or k >= count
        want_d = np.stack([vc.dist(metric, queries[r], x[top[r]]) for r in range(nq)])
        for block in (None, 5):   # the blocks of queries change nothing
            assert vc.check_batch(metric, ids, x, queries, k, ids[top], want_d, 1e-12, rows_per_block=block) == ties
        if k > 1:   # ... and it does reject: two entries swapped, a wrong id, a distance off by more than the bound
            swapped = ids[top].copy()
            swapped[7, [0, 1]] = swapped[7, [1, 0]]
            with pytest.raises(AssertionError, match="query 7, place 0"):
                vc.check_batch(metric, ids, x, queries, k, swapped, want_d, 1e-12, rows_per_block=5)
        if k < count:
            wrong = ids[top].copy()
            wrong[22, -1] = ids[np.setdiff1d(np.arange(count), top[22])[0]]
            with pytest.raises(AssertionError, match="query 22"):
                vc.check_batch(metric, ids, x, queries, k, wrong, want_d, 1e-12)
        off = want_d.copy()
        off[3, 0] += 1e-9 * max(1.0, abs(off[3, 0]))
        with pytest.raises(AssertionError, match="query 3, place 0: distance"):
            vc.check_batch(metric, ids, x, queries, k, ids[top], off, 1e-12)
    with pytest.raises(AssertionError):
        vc.batch_keys(metric, queries + np.float32(0.5), x)


def test_generators_are_reproducible():
    a, qa = vc.float_store(50, 7, 3)
    b, qb = vc.float_store(50, 7, 3)
    assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(qa, qb)
    assert np.array_equal(a, np.random.default_rng(7).uniform(-1, 1, size=(50, 7)).astype(np.float32))
    ids = vc.scattered_ids(np.random.default_rng(1), 40)
    assert len(set(ids.tolist())) == 40 and ids.dtype == np.uint64
