"""CPU checker of harmonic centrality by HyperBall for the harmonic tests (numpy only).  The rules are those of include/fgpu.h
(fgpu_harmonic): every vertex carries a HyperLogLog sketch of 1024 one-byte registers; C_0[v] holds v's own (slot, rank) from
the murmur3 finaliser of its row index; iteration t takes C_t[v] = the bytewise max of C_{t-1}[v] and of C_{t-1}[w] over the
stored entries (v, w) of row v; a vertex whose sketch changed adds (count(C_t[v]) - est_{t-1}[v]) / t to its score; the run ends
after the first iteration that changes no sketch.  tests/test_hc_cpu.py holds it against a per-vertex restatement and against
plain BFS."""
import math

import numpy as np

M = 1024
ALPHA_MM = 0.7213 / (1 + 1.079 / 1024) * 1024 * 1024
_POW = 2.0 ** -np.arange(256, dtype=np.float64)


def hash_slot_rank(v):
    """(slot, rank) of the vertices v (array or int): the murmur3 32-bit finaliser, slot = the top 10 bits, rank = 1 + the
    leading zeros of the low 22 bits written in 22 bits (23 when they are all zero)"""
    h = np.atleast_1d(np.asarray(v, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    mask = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & mask
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & mask
    h ^= h >> np.uint64(16)
    slot = (h >> np.uint64(22)).astype(np.int64)
    w = (h & np.uint64(0x3FFFFF)).astype(np.int64)
    bits = np.zeros(len(w), dtype=np.int64)                      # bit length of w
    nz = w > 0
    bits[nz] = np.floor(np.log2(w[nz])).astype(np.int64) + 1     # (exact: w < 2^22)
    rank = 23 - bits
    return slot, rank


def count_one(c):
    """the estimate of one sketch (uint8[1024]) -> float"""
    s = float(_POW[c].sum())                                     # exact: dyadic terms >= 2^-23, sum <= 1024
    z = int((c == 0).sum())
    e = ALPHA_MM / s
    if e <= 2560 and z > 0:
        e = 1024 * math.log(1024 / z)
    elif e > 2 ** 32 / 30:
        e = -(2 ** 32) * math.log(1 - e / 2 ** 32)
    return e


def count(C):
    """the estimates of the sketches C (uint8[k, 1024]) -> float64[k]"""
    C = np.asarray(C)
    if len(C) == 0:
        return np.zeros(0, dtype=np.float64)
    s = _POW[C].sum(axis=1)                                      # exact in any order
    z = (C == 0).sum(axis=1)
    e = ALPHA_MM / s
    small = (e <= 2560) & (z > 0)
    large = ~small & (e > 2 ** 32 / 30)
    e[small] = 1024 * np.log(1024 / z[small])
    e[large] = -(2 ** 32) * np.log(1 - e[large] / 2 ** 32)
    return e


def _pattern(n, rowptr, colidx):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    return rows, colidx


def csr_of(n, rows, cols):
    """(rowptr, colidx) of the pattern of the (row, col) pairs, rows sorted, duplicates kept."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


_last = [None, None]   # the last run: harmonic() and round_margin() of one graph share it


def _run(n, rowptr, colidx, active):
    """-> (score, est, registers, stats[0:2]) of the rules, est = the final estimates (NaN outside `active`)"""
    key = (n, np.asarray(rowptr, dtype=np.int64).tobytes(), np.asarray(colidx, dtype=np.int64).tobytes(),
           None if active is None else np.asarray(active, dtype=bool).tobytes())
    if _last[0] != key:
        _last[0], _last[1] = key, _run_rules(n, rowptr, colidx, active)
    score, est, C, st = _last[1]
    return score.copy(), est.copy(), C.copy(), list(st)


def _run_rules(n, rowptr, colidx, active):
    rows, cols = _pattern(n, rowptr, colidx)
    on = np.ones(n, dtype=bool) if active is None else np.asarray(active, dtype=bool)
    keep = on[rows] & on[cols]
    rows, cols = rows[keep], cols[keep]
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    C = np.zeros((n, M), dtype=np.uint8)
    ids = np.flatnonzero(on)
    slot, rank = hash_slot_rank(ids)
    C[ids, slot] = rank.astype(np.uint8)
    est = np.full(n, np.nan)
    est[ids] = count(C[ids])
    score = np.zeros(n, dtype=np.float64)
    iters, changes, t = 0, 0, 0
    starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]]) if len(rows) else np.zeros(0, dtype=np.int64)
    heads = rows[starts] if len(rows) else rows
    while True:
        t += 1
        new = C.copy()
        if len(rows):
            new[heads] = np.maximum(C[heads], np.maximum.reduceat(C[cols], starts, axis=0))
        moved = np.flatnonzero((new != C).any(axis=1))
        if len(moved) == 0:
            break
        e = count(new[moved])
        score[moved] += (e - est[moved]) / t
        est[moved] = e
        C = new
        iters += 1
        changes += len(moved)
    return score, est, C, [iters, changes]


def harmonic(n, rowptr, colidx, active=None):
    """-> (score float64[n], reachable int64[n], registers uint8[n, 1024], the four counters of fgpu_harmonic): [iterations that
    changed a sketch, sketch changes summed over them, the largest reachable, vertices with a non-zero score].  Outside `active`
    the score is 0.0, reachable -1 and the sketch zero."""
    if n == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros((0, M), dtype=np.uint8), [0, 0, 0, 0]
    score, est, C, st = _run(n, rowptr, colidx, active)
    on = ~np.isnan(est)
    reach = np.full(n, -1, dtype=np.int64)
    reach[on] = np.floor(est[on] + 0.5).astype(np.int64) - 1     # llround of a positive value
    return score, reach, C, st + [int(max(reach.max(), 0)), int((score != 0).sum())]


def round_margin(n, rowptr, colidx, active=None):
    """the smallest |est_final - floor(est_final) - 0.5| over the active vertices (inf when there is none): how far the final
    estimates are from the point at which llround flips"""
    if n == 0:
        return math.inf
    est = _run(n, rowptr, colidx, active)[1]
    est = est[~np.isnan(est)]
    return float(np.abs(est - np.floor(est) - 0.5).min()) if len(est) else math.inf


def exact_harmonic(n, rowptr, colidx, active=None):
    """plain BFS from every vertex -> (sum over the reached w != v of 1 / d(v, w), the number of them); 0 / -1 outside `active`"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    on = np.ones(n, dtype=bool) if active is None else np.asarray(active, dtype=bool)
    score = np.zeros(n, dtype=np.float64)
    reach = np.full(n, -1, dtype=np.int64)
    for s in np.flatnonzero(on):
        seen = np.zeros(n, dtype=bool)
        seen[s] = True
        front = np.array([s], dtype=np.int64)
        d, total, cnt = 0, 0.0, 0
        while len(front):
            d += 1
            lo, ln = rowptr[front], rowptr[front + 1] - rowptr[front]
            total_len = int(ln.sum())
            if total_len == 0:
                break
            # the entries of the frontier's rows: position k of the concatenation is lo[row of k] + (k - start of that row)
            start = np.cumsum(ln) - ln
            nb = colidx[np.repeat(lo - start, ln) + np.arange(total_len)]
            nb = np.unique(nb[on[nb] & ~seen[nb]])
            seen[nb] = True
            total += len(nb) / d
            cnt += len(nb)
            front = nb
        score[s], reach[s] = total, cnt
    return score, reach
