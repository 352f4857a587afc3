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


def test_generators_are_reproducible():
    a, qa = vc.float_store(50, 7, 3)
    b, qb = vc.float_store(50, 7, 3)
    assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(qa, qb)
    assert np.array_equal(a, np.random.default_rng(7).uniform(-1, 1, size=(50, 7)).astype(np.float32))
    ids = vc.scattered_ids(np.random.default_rng(1), 40)
    assert len(set(ids.tolist())) == 40 and ids.dtype == np.uint64
