"""CPU checker of weakly connected components for the WCC tests (numpy only): min-label propagation over both directions
of every stored entry plus pointer jumping, iterated to a fixed point.  label[v] = the smallest vertex id of v's component —
what fgpu_wcc returns — and -1 outside `active`.  tests/test_wcc_cpu.py holds it against a plain union-find."""
import numpy as np


def csr_of(n, rows, cols):
    """(rowptr, colidx) of the pattern of the (row, col) pairs, rows sorted, duplicates kept."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


def _row_min(n, rowptr, colidx, label):
    """min over the labels of every row's entries (n for an empty row)"""
    out = np.full(n, n, dtype=np.int64)
    if len(colidx) == 0:
        return out
    deg = np.diff(rowptr)
    nz = np.flatnonzero(deg)
    out[nz] = np.minimum.reduceat(label[colidx], rowptr[nz])
    return out


def wcc_labels(n, rowptr, colidx, active=None):
    """Components of the undirected view of the CSR pattern (rowptr, colidx); `active` (bool[n], optional) restricts the
    run to the induced subgraph of the flagged vertices."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    if active is not None:
        active = np.asarray(active, dtype=bool)
        keep = active[rows] & active[colidx]
        rows, colidx = rows[keep], colidx[keep]
    # the out-view and the in-view of the kept entries, each as a CSR
    fwd_p, fwd_c = csr_of(n, rows, colidx)
    bwd_p, bwd_c = csr_of(n, colidx, rows)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = np.minimum(label, np.minimum(_row_min(n, fwd_p, fwd_c, label), _row_min(n, bwd_p, bwd_c, label)))
        while True:   # pointer jumping: label[v] is a vertex of v's component with a smaller id
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            break
        label = new
    if active is not None:
        label[~active] = -1
    return label


def union_find_labels(n, rows, cols, active=None):
    """The same labels by a plain Python union-find (small graphs only)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for r, c in zip(rows, cols):
        r, c = int(r), int(c)
        if active is not None and not (active[r] and active[c]):
            continue
        a, b = find(r), find(c)
        if a != b:
            parent[max(a, b)] = min(a, b)
    out = np.array([find(v) for v in range(n)], dtype=np.int64)
    if active is not None:
        out[~np.asarray(active, dtype=bool)] = -1
    return out


def components(label):
    """number of components among the labelled (>= 0) vertices"""
    label = np.asarray(label)
    return int((label == np.arange(len(label))).sum())
