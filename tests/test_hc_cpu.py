"""CPU: the harmonic-centrality checker of tests/hc_check.py (the rules of include/fgpu.h, fgpu_harmonic) — the hash on pinned
values, the vectorised checker against a per-vertex pure-Python restatement, and the accuracy of the rules themselves against
plain BFS: for every vertex with an exact score > 0 the relative error stays within 3 x 1.04 / sqrt(1024) = 0.0975, three
standard errors of a 1024-register HyperLogLog."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hc_check import ALPHA_MM, count, count_one, csr_of, exact_harmonic, harmonic, hash_slot_rank, round_margin  # noqa: E402

BOUND = 3 * 1.04 / math.sqrt(1024)


def murmur(v):
    h = v & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def slot_rank(v):
    h = murmur(v)
    w = h & 0x3FFFFF
    return h >> 22, (23 if w == 0 else 22 - w.bit_length() + 1)


def test_hash_pinned_values():
    assert slot_rank(0) == (0, 23)
    # the murmur3 finaliser's published vectors: fmix32(1) = 0x514E28B7, fmix32(0xFFFFFFFF) = 0x81F16F39
    assert murmur(1) == 0x514E28B7 and murmur(0xFFFFFFFF) == 0x81F16F39
    assert slot_rank(1) == (0x514E28B7 >> 22, 22 - (0x514E28B7 & 0x3FFFFF).bit_length() + 1) == (325, 3)   # w = 0x0E28B7: 20 bits, two leading zeros
    ids = np.array([0, 1, 2, 3, 199, 4098, 2 ** 31, 2 ** 32 - 2], dtype=np.uint64)
    slot, rank = hash_slot_rank(ids)
    assert [(int(s), int(r)) for s, r in zip(slot, rank)] == [slot_rank(int(v)) for v in ids]
    assert ((rank >= 1) & (rank <= 23)).all() and ((slot >= 0) & (slot < 1024)).all()
    # a bijection: no two of the first 2^16 ids share (slot, low bits)
    s, r = hash_slot_rank(np.arange(1 << 16))
    assert len({murmur(v) for v in range(1 << 12)}) == 1 << 12
    assert s.max() == 1023 and r.max() <= 23


def test_count_branches():
    one = np.zeros(1024, dtype=np.uint8)
    one[5] = 3
    assert count_one(one) == 1024 * math.log(1024 / 1023)                   # the small-range correction
    assert abs(count_one(one) - 1.0005) < 1e-4
    full = np.full(1024, 4, dtype=np.uint8)                                   # no zero register: the raw estimator
    assert count_one(full) == ALPHA_MM / (1024 * 2.0 ** -4)
    assert count_one(full) > 2560
    both = np.stack([one, full])
    assert np.allclose(count(both), [count_one(one), count_one(full)], rtol=0, atol=1e-9)


def python_harmonic(n, rows, cols, active=None):
    """the rules vertex by vertex, in plain Python"""
    on = [True] * n if active is None else [bool(x) for x in active]
    nbr = [set() for _ in range(n)]
    for r, c in zip(rows, cols):
        if on[int(r)] and on[int(c)]:
            nbr[int(r)].add(int(c))
    C = [[0] * 1024 for _ in range(n)]
    est = [0.0] * n
    score = [0.0] * n
    for v in range(n):
        if on[v]:
            s, r = slot_rank(v)
            C[v][s] = r
            est[v] = count_one(np.array(C[v], dtype=np.uint8))
    t, iters, changes = 0, 0, 0
    while True:
        t += 1
        new, moved = [], 0
        for v in range(n):
            row = list(C[v])
            for w in nbr[v]:
                row = [max(a, b) for a, b in zip(row, C[w])]
            new.append(row)
        for v in range(n):
            if new[v] != C[v]:
                e = count_one(np.array(new[v], dtype=np.uint8))
                score[v] += (e - est[v]) / t
                est[v] = e
                moved += 1
        if moved == 0:
            break
        C = new
        iters += 1
        changes += moved
    reach = [int(math.floor(est[v] + 0.5)) - 1 if on[v] else -1 for v in range(n)]
    return np.array(score), np.array(reach, dtype=np.int64), np.array(C, dtype=np.uint8), [iters, changes]


@pytest.mark.parametrize("seed", range(4))
def test_checker_matches_the_per_vertex_restatement(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 40))
    m = int(rng.integers(0, 3 * n))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)                 # duplicates and self-loops included
    active = None if seed % 2 == 0 else rng.random(n) < 0.7
    score, reach, regs, st = harmonic(n, *csr_of(n, rows, cols), active)
    ws, wr, wc, wst = python_harmonic(n, rows, cols, active)
    assert np.array_equal(regs, wc)
    assert st[:2] == wst and np.array_equal(reach, wr)
    assert np.abs(score - ws).max() <= 1e-9
    assert st[2] == max(int(reach.max()), 0) and st[3] == int((score != 0).sum())
    if active is not None:
        assert (score[~active] == 0).all() and (reach[~active] == -1).all() and not regs[~active].any()


def graphs():
    yield "path", 4, [0, 1, 2], [1, 2, 3]
    yield "star", 6, [0] * 5, [1, 2, 3, 4, 5]
    a = np.arange(200)
    r = np.concatenate([a[:-1], a[:-7]])
    yield "test08", 200, r, np.concatenate([a[1:], a[7:]])
    rng = np.random.default_rng(7)
    yield "random1000", 1000, rng.integers(0, 1000, 3000), rng.integers(0, 1000, 3000)
    yield "random4096", 4096, rng.integers(0, 4096, 16000), rng.integers(0, 4096, 16000)


@pytest.mark.parametrize("name,n,rows,cols", list(graphs()), ids=[g[0] for g in graphs()])
def test_accuracy_of_the_rules_against_plain_bfs(name, n, rows, cols):
    rp, ci = csr_of(n, rows, cols)
    score, reach, _, st = harmonic(n, rp, ci)
    exact, ereach = exact_harmonic(n, rp, ci)
    pos = exact > 0
    err = np.abs(score[pos] - exact[pos]) / exact[pos]
    rerr = np.abs(reach[pos] - ereach[pos]) / ereach[pos]
    print(name, "largest relative error: score", float(err.max()), "reachable", float(rerr.max()))
    assert err.max() <= BOUND
    assert rerr.max() <= BOUND
    # a vertex without an out-entry scores exactly 0.0 and reaches nobody
    sink = np.diff(rp) == 0
    assert (score[sink] == 0.0).all() and (reach[sink] == 0).all()
    if name in ("path", "star"):
        assert np.array_equal(reach, ereach)
    if name == "test08":
        assert int(np.argmax(score)) == 0 and (score[0] > score[1:]).all()
        assert score[199] == 0.0


def test_round_margin_and_the_empty_graph():
    rp, ci = csr_of(4, [0, 1, 2], [1, 2, 3])
    m = round_margin(4, rp, ci)
    assert 0 < m <= 0.5
    score, reach, regs, st = harmonic(0, [0], [])
    assert len(score) == 0 and regs.shape == (0, 1024) and st == [0, 0, 0, 0]
    score, reach, regs, st = harmonic(1, [0, 1], [0])                        # a self-loop alone changes nothing
    assert score.tolist() == [0.0] and reach.tolist() == [0] and st == [0, 0, 0, 0]
