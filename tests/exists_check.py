"""The contract of fgpu_expand_exists in numpy (test_exists_check_cpu.py pins it, test_gpu_expand_exists.py holds the device to it).

expected(): bit i = row i of the chain's result is not empty — chain_graph.reference, that is oracle.delta_lmxm hop by hop and the
label filter at the end.

decide(): the device's decision rule, restated.  The last hop's rule is the row-level mask R_i = ((F·m)<not (F·dm)> U (F·dp)) &
label, so with D = the columns that occur in the last dm, P[u] = "u has a label-passing dp entry, or a label-passing m entry
outside D", Q[u] = "u has a label-passing m entry inside D": rows whose last frontier holds a P vertex are sure, rows that hold
only Q vertices are undecided (stats[1] counts them) and take the exact pass.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_graph as cg  # noqa: E402

U64, I64 = np.uint64, np.int64
SKIP = cg.SKIP


def rows_nonempty(c):
    return np.diff(np.asarray(c.rowptr).astype(I64)) > 0


def expected(src, layers, n, label=None):
    """label: the ids that pass, or None.  n: the vertices the sources name (a last layer may have another column count: the
    label is then applied here, to the same effect)."""
    if layers[-1][0].ncols == n:
        return rows_nonempty(cg.reference(src, layers, n, label)[0])
    rows, cols = cg.reference(src, layers, n)[0].pairs()
    if label is not None:
        rows = rows[np.isin(cols, label)]
    out = np.zeros(len(src), dtype=bool)
    out[rows.astype(I64)] = True
    return out


def decide(src, layers, n, label=None):
    """(sure, undecided) per row, from the frontier before the last hop."""
    fr = cg.reference(src, layers[:-1], n)[0]
    m, dp, dm = layers[-1]
    ok = np.ones(m.ncols, dtype=bool)
    if label is not None:
        ok[:] = False
        ok[np.asarray(label).astype(I64)] = True
    in_d = np.zeros(m.ncols, dtype=bool)
    if dm is not None and dm.nnz:
        in_d[dm.colidx.astype(I64)] = True
    p = np.zeros(m.nrows, dtype=bool)
    q = np.zeros(m.nrows, dtype=bool)
    rows, cols = (x.astype(I64) for x in m.pairs())
    good = ok[cols]
    p[rows[good & ~in_d[cols]]] = True
    q[rows[good & in_d[cols]]] = True
    if dp is not None and dp.nnz:
        rows, cols = (x.astype(I64) for x in dp.pairs())
        p[rows[ok[cols]]] = True
    k = len(src)
    sure = np.zeros(k, dtype=bool)
    maybe = np.zeros(k, dtype=bool)
    frows, fcols = (x.astype(I64) for x in fr.pairs())
    sure[frows[p[fcols]]] = True
    maybe[frows[q[fcols]]] = True
    return sure, maybe & ~sure


def row_lengths(src, layer, n):
    """Summed lengths of the source vertices' m, dp and dm rows (what a one-hop call may read at the most)."""
    tot = 0
    for x in layer:
        if x is None:
            continue
        deg = np.diff(x.rowptr.astype(I64))
        s = np.asarray(src, dtype=U64)
        tot += int(deg[s[s != SKIP].astype(I64)].sum())
    return tot


# ---- the mask quirk by hand, n = 8: s -> u1, s -> u2; the last m = {(u1, v), (u2, v)}, the last dm = {(u2, v)} ------------------
S, U1, U2, V, V2, V3, LONE = 0, 1, 2, 3, 4, 5, 6
MASK_N = 8


def _csr(pairs):
    import oracle
    r = np.array([p[0] for p in pairs], dtype=U64)
    c = np.array([p[1] for p in pairs], dtype=U64)
    return oracle.build_csr(MASK_N, MASK_N, r, c)


def mask_cases():
    """name -> (src, layers, label ids or None, the rows that match, the undecided rows).  Row 0 is s, row 1 is skipped, row 2
    a vertex without out-edges.  A per-edge rule (an entry is live unless dm holds that very entry) calls row 0 of "masked" a
    match through (u1, v); the row-level mask does not."""
    src = np.array([S, SKIP, LONE], dtype=U64)
    hop0 = (_csr([(S, U1), (S, U2)]), None, None)
    base, dm = [(U1, V), (U2, V)], _csr([(U2, V)])
    no_v2_v3 = np.array([0, 1, 2, 3, 6, 7], dtype=U64)
    none, row0 = np.zeros(3, dtype=bool), np.array([True, False, False])
    cases = {
        "masked": (src, [hop0, (_csr(base), None, dm)], None, none, row0),
        "masked, clean twin": (src, [hop0, (_csr(base), None, None)], None, row0, none),
        "plus (u1, v2)": (src, [hop0, (_csr(base + [(U1, V2)]), None, dm)], None, row0, none),
        "plus dp (u2, v3)": (src, [hop0, (_csr(base), _csr([(U2, V3)]), dm)], None, row0, none),
        "plus (u1, v2), label drops v2": (src, [hop0, (_csr(base + [(U1, V2)]), None, dm)], no_v2_v3, none, row0),
        "plus dp (u2, v3), label drops v3": (src, [hop0, (_csr(base), _csr([(U2, V3)]), dm)], no_v2_v3, none, row0),
        # one hop from u1 and from u2: the row of u1 keeps v (no frontier vertex of ITS row is tombstoned), the row of u2 loses it
        "one hop": (np.array([U1, U2, SKIP], dtype=U64), [(_csr(base), None, dm)], None, np.array([True, False, False]),
                    np.array([True, True, False])),
    }
    return cases
