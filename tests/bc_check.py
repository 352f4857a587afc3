"""CPU checker of betweenness centrality for the betweenness tests (numpy + scipy.sparse): batched Brandes in FP64 with
every level vectorised over (vertex, source).  centrality[v] = the sum over `sources` (taken as given: a duplicate counts
twice) of delta_s(v) = sum over out-neighbours w of v with d_s(w) = d_s(v) + 1 of sigma_s(v) / sigma_s(w) * (1 + delta_s(w)),
sigma the number of shortest directed paths, d the BFS depth over the out-edges — what fgpu_betweenness returns.  A source
never scores for itself; the pattern is boolean (duplicate entries and self-loops change nothing); `active` (bool[n],
optional) restricts the run to the induced subgraph of the flagged vertices, the others get 0.  tests/test_bc_cpu.py holds it
against networkx."""
import numpy as np
import scipy.sparse as sp


def csr_of(n, rows, cols):
    """(rowptr, colidx) of the boolean pattern of the (row, col) pairs: rows sorted, columns ascending, duplicates dropped."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    if len(rows):
        key = np.unique(rows * max(n, 1) + cols)
        rows, cols = key // max(n, 1), key % max(n, 1)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


def _pattern(n, rowptr, colidx, active):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    if active is not None:
        keep = active[rows] & active[colidx]
        rows, colidx = rows[keep], colidx[keep]
    a = sp.csr_matrix((np.ones(len(rows)), (rows, colidx)), shape=(n, n))
    a.sum_duplicates()
    a.data[:] = 1.0
    a.sort_indices()
    return a


def _batch(a, n, src):
    """one batch of sources: the dependency matrix delta (n x len(src))"""
    b = len(src)
    cols = np.arange(b)
    depth = np.full((n, b), -1, dtype=np.int32)
    sigma = np.zeros((n, b))
    depth[src, cols] = 0
    sigma[src, cols] = 1.0
    d = 0
    while True:
        fr = np.flatnonzero((depth == d).any(axis=1))          # vertices in some source's frontier
        if len(fr) == 0:
            break
        x = np.where(depth[fr] == d, sigma[fr], 0.0)
        y = a[fr].T @ x                                           # y[w, k] = sum over frontier in-neighbours u of sigma[u, k]
        new = (depth == -1) & (y > 0)
        if not new.any():
            break
        depth[new] = d + 1
        sigma[new] = y[new]
        d += 1
    deepest = d
    delta = np.zeros((n, b))
    for d in range(deepest - 1, 0, -1):
        rows = np.flatnonzero((depth == d).any(axis=1))
        if len(rows) == 0:
            continue
        nxt = depth == d + 1
        w = np.zeros((n, b))
        w[nxt] = (1.0 + delta[nxt]) / sigma[nxt]
        s = a[rows] @ w                                           # row order: the sum over out-neighbours at depth d + 1
        here = depth[rows] == d
        delta[rows] = np.where(here, sigma[rows] * s, delta[rows])
    return delta, deepest


def betweenness(n, rowptr, colidx, sources, active=None, batch=16):
    """unnormalised betweenness over `sources`; returns (centrality float64[n], deepest level over all batches)"""
    if active is not None:
        active = np.asarray(active, dtype=bool)
    sources = np.asarray(sources, dtype=np.int64)
    cent = np.zeros(n)
    deepest = 0
    if n == 0 or len(sources) == 0:
        return cent, deepest
    a = _pattern(n, rowptr, colidx, active)
    for first in range(0, len(sources), batch):
        delta, dp = _batch(a, n, sources[first:first + batch])
        deepest = max(deepest, dp)
        for k in range(delta.shape[1]):                           # lanes in source order, batches in sequence
            cent += delta[:, k]
    if active is not None:
        cent[~active] = 0.0
    return cent, deepest
