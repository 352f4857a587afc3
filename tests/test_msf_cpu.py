"""CPU only: the Kruskal checker of tests/msf_check.py against an independent Boruvka in plain Python, on small random graphs
whose weights are drawn from a handful of values so that ties dominate, and the key K on hand-written bit patterns."""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of, components, key_of, msf  # noqa: E402

U64 = np.uint64
WEIGHTS = [1.0, 2.0, -0.0, 0.0, -3.5, math.inf, -math.inf]


def py_key(w):
    """K in plain Python integers"""
    b = struct.unpack("<Q", struct.pack("<d", w))[0]
    if b == 1 << 63:
        b = 0
    return b ^ ((1 << 64) - 1) if b >> 63 else b ^ (1 << 63)


def boruvka(n, pairs):
    """pairs: {(lo, hi): weight}.  Rounds of: every component picks its smallest outgoing edge by (K, lo, hi); all picked edges
    are added at once (the order is strict, so they close no cycle)."""
    comp = list(range(n))
    forest = set()
    while True:
        best = {}
        for (lo, hi), w in pairs.items():
            a, b = comp[lo], comp[hi]
            if a == b:
                continue
            k = (py_key(w), lo, hi)
            for c in (a, b):
                if c not in best or k < best[c]:
                    best[c] = k
        if not best:
            break
        for _, lo, hi in set(best.values()):
            forest.add((lo, hi))
            a, b = comp[lo], comp[hi]
            if a != b:
                new, old = min(a, b), max(a, b)
                comp = [new if c == old else c for c in comp]
    return sorted(forest), comp


def test_kruskal_checker_equals_boruvka_on_tied_weights():
    rng = np.random.default_rng(20240611)
    for _ in range(200):
        n = int(rng.integers(2, 71))
        m = int(rng.integers(0, 3 * n))
        pairs = {}
        for _ in range(m):
            a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
            if a != b:
                pairs[(min(a, b), max(a, b))] = WEIGHTS[int(rng.integers(0, len(WEIGHTS)))]
        lo = np.array([p[0] for p in pairs], dtype=np.int64)
        hi = np.array([p[1] for p in pairs], dtype=np.int64)
        w = np.array([pairs[p] for p in pairs], dtype=np.float64)
        rows, cols = np.concatenate([lo, hi, np.arange(n)]), np.concatenate([hi, lo, np.arange(n)])   # + a full diagonal
        bits = np.concatenate([bits_of(w), bits_of(w), bits_of(np.full(n, -9.0))])
        fr, fc, fb, comp = msf(n, rows, cols, bits)
        want, wcomp = boruvka(n, pairs)
        assert list(zip(fr.tolist(), fc.tolist())) == want
        assert comp.tolist() == wcomp
        assert len(fr) == n - components(comp)
        assert [struct.unpack("<Q", struct.pack("<d", pairs[p]))[0] for p in want] == fb.tolist()


def test_key_order_on_bit_patterns():
    def k(b):
        return int(key_of(np.array([b], dtype=U64))[0])

    neg_nan, neg_inf, neg35 = 0xFFF8000000000001, 0xFFF0000000000000, 0xC00C000000000000
    neg_zero, zero, sub, one = 0x8000000000000000, 0x0, 0x1, 0x3FF0000000000000
    pos_inf, pos_nan = 0x7FF0000000000000, 0x7FF8000000000000
    assert k(neg_zero) == k(zero)
    chain = [neg_nan, neg_inf, neg35, zero, sub, one, pos_inf, pos_nan]
    keys = [k(b) for b in chain]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert struct.unpack("<d", struct.pack("<Q", neg35))[0] == -3.5
    for b in chain[1:-1] + [neg_zero]:   # (the numbers: a NaN's payload need not survive a trip through a Python float)
        assert k(b) == py_key(struct.unpack("<d", struct.pack("<Q", b))[0])
    assert k(0x7FFFFFFFFFFFFFFF) == 0xFFFFFFFFFFFFFFFF and k(0xFFFFFFFFFFFFFFFF) == 0


def test_active_subset_and_bool_matrix():
    rows = np.array([0, 1, 1, 2, 2, 3, 0, 3])
    cols = np.array([1, 0, 2, 1, 3, 2, 3, 0])
    fr, fc, fb, comp = msf(4, rows, cols)   # a 4-cycle, every weight 1.0: the largest pair (2, 3) stays out
    assert list(zip(fr.tolist(), fc.tolist())) == [(0, 1), (0, 3), (1, 2)]
    assert set(fb.tolist()) == {0x3FF0000000000000} and comp.tolist() == [0, 0, 0, 0]
    fr, fc, fb, comp = msf(4, rows, cols, active=np.array([True, False, True, True]))
    assert list(zip(fr.tolist(), fc.tolist())) == [(0, 3), (2, 3)] and comp.tolist() == [0, -1, 0, 0]
