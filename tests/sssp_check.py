"""Checker for fgpu_sssp (no GPU, no engine import): the rules of include/fgpu.h restated in plain Python / numpy.

sssp(n, rows, cols, bits, src) -> (dist float64[n], parent int64[n], depth int64[n])
  dist    a binary-heap Dijkstra with lazy deletion; a path's weights are added left to right from the source in FP64, a sum
          that is not finite is skipped, the diagonal is ignored, -0.0 is 0.0.  +inf where no route reaches.
  depth   the BFS depth from src over the TIGHT entries alone ((u, v), u != v, dist[u] + w finite and == dist[v]); -1 unreached.
  parent  the smallest u with (u, v) tight and depth[u] + 1 == depth[v]; parent[src] = src, -1 unreached.
bits None = a BOOL matrix, every weight 1.0; otherwise one binary64 bit pattern per entry (bits_of of msf_check)."""
import heapq

import numpy as np

U64 = np.uint64


def weights_of(bits, m):
    if bits is None:
        return np.ones(m, dtype=np.float64)
    w = np.ascontiguousarray(bits, dtype=U64).view(np.float64).copy()
    if np.isnan(w).any() or (np.signbit(w) & (w != 0.0)).any():
        raise ValueError("a weight is NaN or negative")
    return w + 0.0   # -0.0 + 0.0 = +0.0


def csr_of(n, rows, cols, w):
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    rows, cols, w = rows[order], cols[order], w[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), rows, cols, w


def dijkstra(n, rowptr, cols, w, src):
    dist = [float("inf")] * n
    dist[src] = 0.0
    rp, cl, wl = rowptr.tolist(), cols.tolist(), w.tolist()
    heap = [(0.0, src)]
    inf = float("inf")
    while heap:
        d, u = heapq.heappop(heap)
        if d != dist[u]:
            continue   # lazy deletion
        for k in range(rp[u], rp[u + 1]):
            v = cl[k]
            nd = d + wl[k]
            if v != u and nd < inf and nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, v))
    return np.array(dist, dtype=np.float64)


def tight_tree(n, rows, cols, w, dist, src):
    """(parent, depth) of the rule above from dist and the entries"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = dist[rows] + w
    tight = (rows != cols) & np.isfinite(s) & (s == dist[cols])
    tr, tc = rows[tight], cols[tight]
    depth = np.full(n, -1, dtype=np.int64)
    parent = np.full(n, -1, dtype=np.int64)
    depth[src] = 0
    parent[src] = src
    level = 0
    while True:
        push = (depth[tr] == level) & (depth[tc] == -1)
        if not push.any():
            break
        new = np.unique(tc[push])
        depth[new] = level + 1
        best = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(best, tc[push], tr[push])
        parent[new] = best[new]
        level += 1
    return parent, depth


def sssp(n, rows, cols, bits, src):
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    w = weights_of(bits, len(rows))
    rowptr, rows, cols, w = csr_of(n, rows, cols, w)
    dist = dijkstra(n, rowptr, cols, w, src)
    parent, depth = tight_tree(n, rows, cols, w, dist, src)
    return dist, parent, depth
