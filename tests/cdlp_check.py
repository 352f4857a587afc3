"""CPU checker of community detection by label propagation for the CDLP tests (numpy only).  The rules are those of
include/fgpu.h (fgpu_cdlp): label_0[v] = v; iteration t computes every label from label_{t-1} only; a row's new label is the
most frequent label among its stored entries (each entry votes once, a diagonal entry like any other, an entry whose column is
inactive not at all), ties to the smallest label; a row without a voting entry keeps its label; the run ends after itermax
iterations or after the first iteration that changes nothing.  tests/test_cdlp_cpu.py holds it against a dict-counting
version."""
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


def pattern(n, rowptr, colidx):
    """the (row, col) pairs of the CSR with duplicates dropped: the matrix is a boolean pattern"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    if len(rows) == 0:
        return rows, colidx
    key = np.unique(rows * n + colidx)
    return key // n, key % n


def cdlp_labels(n, rowptr, colidx, itermax, active=None):
    """-> (labels int64[n] with -1 outside `active`, iterations run, labels changed in the last iteration run)"""
    rows, cols = pattern(n, rowptr, colidx)
    if active is not None:
        active = np.asarray(active, dtype=bool)
        keep = active[rows] & active[cols]
        rows, cols = rows[keep], cols[keep]
    label = np.arange(n, dtype=np.int64)
    iters, changed = 0, 0
    for _ in range(itermax):
        new = label.copy()
        if len(rows):
            votes = label[cols]
            order = np.lexsort((votes, rows))
            r, l = rows[order], votes[order]
            head = np.ones(len(r), dtype=bool)
            head[1:] = (r[1:] != r[:-1]) | (l[1:] != l[:-1])
            at = np.flatnonzero(head)
            length = np.diff(np.append(at, len(r)))
            rr, ll = r[at], l[at]
            best = np.lexsort((ll, -length, rr))              # per row: the longest run first, then the smallest label
            rr, ll = rr[best], ll[best]
            first = np.ones(len(rr), dtype=bool)
            first[1:] = rr[1:] != rr[:-1]
            new[rr[first]] = ll[first]
        changed = int((new != label).sum())
        label = new
        iters += 1
        if changed == 0:
            break
    if active is not None:
        label[~active] = -1
    return label, iters, changed


def cdlp_stats(n, rowptr, colidx, itermax, active=None):
    """-> (labels, the four counters of fgpu_cdlp): [iterations run, labels changed in the last iteration, stored entries of
    the active rows x iterations, distinct labels among the active vertices]"""
    label, iters, changed = cdlp_labels(n, rowptr, colidx, itermax, active)
    rows, _ = pattern(n, rowptr, colidx)
    entries = len(rows) if active is None else int(np.asarray(active, dtype=bool)[rows].sum())
    return label, [iters, changed, iters * entries, len(np.unique(label[label >= 0]))]


def dict_labels(n, rows, cols, itermax, active=None):
    """The same labels by plain Python dict counting (small graphs only)."""
    pairs = sorted(set(zip((int(r) for r in rows), (int(c) for c in cols))))
    on = [True] * n if active is None else [bool(x) for x in active]
    label = list(range(n))
    iters, changed = 0, 0
    for _ in range(itermax):
        counts = [dict() for _ in range(n)]
        for r, c in pairs:
            if on[r] and on[c]:
                counts[r][label[c]] = counts[r].get(label[c], 0) + 1
        new = list(label)
        for v in range(n):
            if counts[v]:
                top = max(counts[v].values())
                new[v] = min(l for l, k in counts[v].items() if k == top)
        changed = sum(1 for v in range(n) if new[v] != label[v])
        label = new
        iters += 1
        if changed == 0:
            break
    out = np.array(label, dtype=np.int64)
    if active is not None:
        out[~np.asarray(active, dtype=bool)] = -1
    return out, iters, changed
