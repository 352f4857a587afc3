"""Graphs built to send a BFS or a vxm down one named path of bfs.hip, and plain numpy references for both.

Pure numpy, deterministic, no code shared with the device or with `oracle` (tests/test_bfs_cases_cpu.py holds the
references to the oracle and the builders to what their rows below claim; tests/test_gpu_bfs_edges.py runs them on the
device).  Every builder returns (n, rows, cols, named): the edge list unique and sorted by (row, col) as int64, and a
dict of the vertices a test names."""
from functools import lru_cache

import numpy as np

# The kernel constants the cases are built around.  Their homes: bfs.hip (QGATE, PULL_QGATE, PUSH_VPB, TINY_*, PULL_H,
# PULL_R, and the padding of a vxm's bitmaps), common.hpp (HUB_DEG, PUSH_HUB_DEG, PUSH_HUB_CHUNK, HYPER_MIN_ROWS), dist.hip
# (fgpu_slab_layout: the padding of a plan's bitmaps).  tests/test_bfs_cases_cpu.py reads the sources and fails, naming the
# case to rebuild, when one of them is retuned.
QGATE = 1 << 17          # a level appends its discoveries to the queue when it can find at most this many: a push that examines
                         # so many edges, a pull with so many vertices unvisited
PULL_QGATE = 1 << 12     # ... or a pull with at most this many unvisited vertices that have an in-edge (bfs_alive_rule)
PUSH_VPB = 1024          # vertices per bitmap-mode push item
PUSH_HUB_DEG = 1024      # out-degree from which a fused push level expands a row from the static chunk list
PUSH_HUB_CHUNK = 1024    # edges per item of that list
HUB_DEG = 4096           # in-degree from which the hub section of a pull level owns a row
TINY_VERTS = 1024        # a queue-mode push level of at most this many vertices and
TINY_EDGES = 4096        # this many edges is run by bfs_tiny_kernel
PULL_H = 1               # in-neighbours of a row kept in the plan's head array
PULL_R = 4               # 64-row words per wavefront trip of a pull level
PAD = 4096               # bitmaps are padded to a multiple of this many vertices
HYPER_MIN_ROWS = 4096    # fgpu_mat_from_coo stores more rows than this hypersparse when at most 1 / 16 of them are populated

RAGGED_SIZES = (1, 2, 3, 63, 64, 65, 255, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4099)
RAGGED_FULL = tuple(n for n in RAGGED_SIZES if n > 3)   # the sizes at which every named vertex of ragged_random exists
PULL_DEGS = (1, 2, 3, 5, 6, 7, 69, 70, 133, 4095, 4096, 4097)
PUSH_DEGS = (1023, 1024, 1025, 2049, 4095, 4096, 4097)
FANS = ((1024, 4), (1025, 4), (1024, 5))


# ---- references -------------------------------------------------------------------------------------------------------

def _finish(n, rows, cols):
    """The edge list without duplicates, ascending by (row, col)."""
    key = np.unique(np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64))
    return n, key // n, key % n


def _case(n, rows, cols, named):
    """What a builder returns: the finished edge list and the named vertices, every array read-only (the builders are
    cached: their arrays are shared by all the tests of a session)."""
    n, rows, cols = _finish(n, rows, cols)
    for x in [rows, cols] + [v for v in named.values() if isinstance(v, np.ndarray)]:
        x.setflags(write=False)
    return n, rows, cols, named


def csr(n, rows, cols):
    """(rowptr, colidx) of the edge list, column ids ascending inside a row, duplicates dropped."""
    _, r, c = _finish(n, rows, cols)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, c


def coo_is_hyper(n, rows):
    """Would fgpu_mat_from_coo store these rows hypersparse?  (A BFS plan takes the dense form only.)"""
    return n > HYPER_MIN_ROWS and len(np.unique(np.asarray(rows))) * 16 <= n


def bfs_levels(n, rows, cols, src, max_level=-1):
    """Frontier-at-a-time BFS.  Returns (level int32[n], edges_traversed): -1 for an unreached vertex; the out-degrees of
    every vertex that entered a frontier, summed (the frontier at max_level is counted and not expanded)."""
    rowptr, col = csr(n, rows, cols)
    deg = np.diff(rowptr)
    level = np.full(n, -1, dtype=np.int32)
    level[src] = 0
    frontier = np.array([src], dtype=np.int64)
    edges, depth = 0, 0
    while len(frontier):
        edges += int(deg[frontier].sum())
        if 0 <= max_level <= depth:
            break
        out = np.concatenate([col[rowptr[v]:rowptr[v + 1]] for v in frontier.tolist()] + [np.zeros(0, dtype=np.int64)])
        frontier = np.unique(out[level[out] < 0])
        depth += 1
        level[frontier] = depth
    return level, edges


def level_steps(level, max_level=-1):
    """Level steps a search takes (what fgpu_bfs_stats calls `levels`): one per frontier it expands — every non-empty one,
    the last of which finds nothing, or max_level of them when the search is cut there first."""
    deepest = int(level.max())
    return deepest + 1 if max_level < 0 or deepest < max_level else max_level


def vxm_bits(n, rows, cols, f_bits, mask_bits=None):
    """OR of the out-neighbours of the set bits of f, and-not mask: (n + 63) // 64 little-endian u64 words, no bit at or
    past n."""
    _, r, c = _finish(n, rows, cols)
    f = ids_of(f_bits, n)
    on = np.zeros(n, dtype=bool)
    on[f] = True
    hit = np.zeros(n, dtype=bool)
    hit[c[on[r]]] = True
    if mask_bits is not None:
        hit[ids_of(mask_bits, n)] = False
    return bits_of(n, np.nonzero(hit)[0])


def bits_of(n, ids):
    b = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    b[np.asarray(ids, dtype=np.int64)] = 1
    return np.packbits(b, bitorder="little").view("<u8").astype(np.uint64)


def ids_of(bits, n):
    b = np.unpackbits(np.ascontiguousarray(bits, dtype="<u8").view(np.uint8), bitorder="little")
    assert not b[n:].any(), "a bit at or past n"
    return np.nonzero(b[:n])[0]


def check_parents(n, rows, cols, src, level, parent):
    """The parent vector of a search with these levels: the source its own parent, every other reached vertex one level
    below its parent along an edge of the graph, -1 for the unreached, as many parents as reached vertices."""
    level = np.asarray(level).astype(np.int64)
    parent = np.asarray(parent).astype(np.int64)
    assert parent[src] == src
    reached = level >= 0
    assert np.all(parent[~reached] == -1)
    assert int((parent >= 0).sum()) == int(reached.sum())
    v = np.nonzero(reached)[0]
    v = v[v != src]
    p = parent[v]
    assert np.all((p >= 0) & (p < n))
    assert np.all(level[p] + 1 == level[v])
    edges = np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64)
    assert np.all(np.isin(p * n + v, edges)), "a parent edge that the graph does not have"


# ---- case builders ----------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def ragged_random(n, seed=0):
    """About 3 n random directed edges over n vertices, with: a self-loop, a 2-cycle, a vertex without in-edge, one without
    out-edge, an edge into n - 1, and an edge from n - 1 to a vertex nothing else points at.  `sources`: an order in which a
    later search reaches fewer vertices than an earlier one.  At n <= 3 whatever of that fits."""
    if n <= 3:
        edges = {1: [(0, 0)], 2: [(0, 0), (0, 1), (1, 0)], 3: [(0, 0), (0, 1), (1, 0), (1, 2)]}[n]
        r, c = zip(*edges)
        return _case(n, r, c, {"sources": [0, n - 1] if n > 1 else [0]})
    assert n >= 9
    rng = np.random.default_rng(1000 * n + seed)
    no_in, no_out, only_via_last, last = 1, n - 2, n - 3, n - 1
    m = 3 * n
    from_ok = np.setdiff1d(np.arange(n), [no_out])
    to_ok = np.setdiff1d(np.arange(n), [no_in, only_via_last])
    rows = rng.choice(from_ok, m).tolist()
    cols = rng.choice(to_ok, m).tolist()
    rows += [3, 4, 5, 0, 2, last, no_in]
    cols += [3, 5, 4, 2, last, only_via_last, 2]
    named = {"self_loop": 3, "two_cycle": (4, 5), "no_in": no_in, "no_out": no_out, "only_via_last": only_via_last,
             "sources": [0, no_out, last]}
    return _case(n, rows, cols, named)


@lru_cache(maxsize=None)
def heavy_push(n=1203, a=400, b=400):
    """L0 = {0}, L1 = 1 .. a, L2 = the top b ids, L3 = the ids between.  0 -> all of L1, every L1 vertex -> all of L2
    (a b > QGATE edges: that level does not append, so the next one walks the bitmap), L2[i] -> L3[i mod |L3|] and back
    into L1, a sparse ring inside the part of L3 that L2 points at (the rest of L3 has no in-edge)."""
    l1 = np.arange(1, a + 1)
    l2 = np.arange(n - b, n)
    l3 = np.arange(a + 1, n - b)
    assert len(l3) > 0
    hit = min(b, len(l3))
    rows = [np.zeros(a, dtype=np.int64), np.repeat(l1, b), l2, l2, l3[:hit:7]]
    cols = [l1, np.tile(l2, a), l3[np.arange(b) % len(l3)], l1[np.arange(b) % a], l3[(np.arange(hit)[::7] + 1) % hit]]
    named = {"L1": l1, "L2": l2, "L3": l3, "sources": [0, int(l2[-1]), int(l3[1])]}
    return _case(n, np.concatenate(rows), np.concatenate(cols), named)


@lru_cache(maxsize=None)
def pull_ladder(degs=PULL_DEGS):
    """Decoys 1 .. max(degs) - 1 (no in-edge: never reached), then per in-degree d a level-1 vertex x_d, a level-3 vertex u_d
    and, with the highest ids, a destination t_d whose in-neighbours are the first d - 1 decoys and x_d.  0 -> x_d,
    t_d -> u_d.  t_3 is vertex n - 1.  At the level that discovers t_d its only in-neighbour in the frontier is the LAST
    entry of its row, in ascending order and in the hub-first order alike (the decoys have x_d's out-degree or more)."""
    k = len(degs)
    ndec = max(degs) - 1
    x0, u0, t0 = 1 + ndec, 1 + ndec + k, 1 + ndec + 2 * k
    n = t0 + k
    order = [d for d in degs if d != 3] + [3]              # t_3 last: the last row of A'
    x = {d: x0 + i for i, d in enumerate(degs)}
    u = {d: u0 + i for i, d in enumerate(degs)}
    t = {d: t0 + i for i, d in enumerate(order)}
    rows, cols = [], []
    for d in degs:
        rows += [np.arange(1, d), [x[d]], [0], [t[d]]]
        cols += [np.full(d - 1, t[d]), [t[d]], [x[d]], [u[d]]]
    rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])
    cols = np.concatenate([np.asarray(c, dtype=np.int64) for c in cols])
    named = {"x": x, "u": u, "t": t, "decoys": np.arange(1, 1 + ndec), "sources": [0, x[degs[-1]], u[degs[0]]]}
    return _case(n, rows, cols, named)


@lru_cache(maxsize=None)
def push_ladder(degs=PUSH_DEGS, pool=5003, tails=10):
    """0 -> h_k, one per out-degree of `degs`, into overlapping ranges of one pool of targets; every 97th target has one
    further out-edge, into a few tail vertices."""
    k = len(degs)
    p0 = 1 + k
    n = p0 + pool + tails
    assert n % 64 and n % 4 and max(degs) <= pool
    h = {d: 1 + i for i, d in enumerate(degs)}
    rows = [np.zeros(k, dtype=np.int64)]
    cols = [np.arange(1, 1 + k)]
    for i, d in enumerate(degs):
        rows.append(np.full(d, h[d]))
        cols.append(p0 + (611 * i + np.arange(d)) % pool)
    j = np.arange(0, pool, 97)
    rows.append(p0 + j)
    cols.append(p0 + pool + (j // 97) % tails)
    named = {"h": h, "pool": np.arange(p0, p0 + pool), "sources": [0, h[degs[-1]], h[degs[0]], int(p0 + 97)]}
    return _case(n, np.concatenate(rows), np.concatenate(cols), named)


@lru_cache(maxsize=None)
def fan(verts, per, mids=32, far=257):
    """0 -> `mids` vertices, which together reach exactly `verts` vertices (one in-edge each), each of which has `per`
    out-edges to distinct vertices of a further layer of `far`; every fifth of those points at the last vertex."""
    m0, v0, f0 = 1, 1 + mids, 1 + mids + verts
    n = f0 + far + 1
    j = np.arange(verts)
    rows = [np.zeros(mids, dtype=np.int64), m0 + j % mids, np.repeat(v0 + j, per), f0 + np.arange(0, far, 5)]
    cols = [np.arange(m0, m0 + mids), v0 + j, f0 + (np.repeat(j * per, per) + np.tile(np.arange(per), verts)) % far,
            np.full(len(range(0, far, 5)), n - 1)]
    named = {"mids": np.arange(m0, m0 + mids), "layer": v0 + j, "far": np.arange(f0, f0 + far),
             "sources": [0, m0, int(v0 + verts - 1)]}
    return _case(n, np.concatenate(rows), np.concatenate(cols), named)


@lru_cache(maxsize=None)
def pull_gate(m, r=1000, decoys=QGATE + 5):
    """0 -> a -> F (m vertices) ; F[0] -> R[0] ; R, r vertices: a tree R[(j - 1) // 8] -> R[j] plus back edges
    R[j + k] -> R[j], k = 1 .. 3 ; then `decoys` vertices without any edge.  In auto direction the level out of a is a pull
    (m edges against few left to look at).  When the control step opens the queue for it, more than QGATE vertices are
    unvisited — the decoys: the bound on all vertices keeps it shut — and m + r of them have an in-edge: at PULL_QGATE
    the pull appends its discoveries, one past it it does not.  The level out of F, one edge against all of R's
    in-edges, is a push: from the queue the pull filled, or from the bitmap."""
    a, f0, r0 = 1, 2, 2 + m
    n = r0 + r + decoys
    j = np.arange(1, r)
    rows = [[0], np.full(m, a), [f0], r0 + (j - 1) // 8]
    cols = [[a], f0 + np.arange(m), [r0], r0 + j]
    for k in range(1, 4):
        jj = np.arange(0, r - k)
        rows.append(r0 + jj + k)
        cols.append(r0 + jj)
    rows = np.concatenate([np.asarray(x, dtype=np.int64) for x in rows])
    cols = np.concatenate([np.asarray(x, dtype=np.int64) for x in cols])
    named = {"a": a, "F": f0 + np.arange(m), "R": r0 + np.arange(r), "decoys": np.arange(r0 + r, n),
             "sources": [0, int(r0), int(f0 + 1)]}
    return _case(n, rows, cols, named)


PULL_GATES = (PULL_QGATE - 1000, PULL_QGATE - 1000 + 1)   # m at the gate and one past it, with r = 1000


def degenerate():
    """name -> (n, rows, cols, named): searches that end at level 0 or 1, and the nnz == 0 early-outs."""
    return {"n1_empty": _case(1, [], [], {"sources": [0]}),
            "n1_self_loop": _case(1, [0], [0], {"sources": [0]}),
            "n2_one_edge": _case(2, [0], [1], {"sources": [0, 1]}),
            "n65_empty": _case(65, [], [], {"sources": [0, 64, 63]})}
