"""Graphs built to send the whole-graph algorithms (pagerank, wcc, cdlp, harmonic, betweenness, msf, maxflow, sssp, sssp_hops)
over the edges of their row split, of their 64-row words and of their batched read-backs.

Pure numpy, deterministic, no code shared with the device (tests/test_algo_edges_cpu.py holds the builders to what their rows
below claim and the checkers to each other on them; tests/test_gpu_algo_edges.py runs them on the device).  Every edge list is
unique and sorted by (row, col) as int64, every array read-only: the builders are cached and their arrays shared by all the
tests of a session."""
from functools import lru_cache

import numpy as np

U64 = np.uint64

# The kernel constants the cases are built around.  Their homes: common.hpp (HUB_DEG, HUB_CHUNK), wcc.hip (WCC_AUTO_MIN_N),
# pagerank.hip / cdlp.hip / harmonic.hip / sssp.hip / maxflow.hip (the batches).  tests/test_algo_edges_cpu.py reads the sources
# and fails when one of them is retuned.
HUB_DEG = 4096           # a row of at least this many entries is the hub kernels' row
HUB_CHUNK = 4096         # entries per item of a snapshot's hub list
WCC_AUTO_MIN_N = 4096    # wcc_mode 0 picks Afforest from this many vertices
BATCH = 4                # PR_BATCH = CDLP_BATCH = HC_BATCH = SSSP_BATCH: iterations enqueued per read-back; forest_compress: four
                         # launches per read-back
MF_BATCH = 16            # maxflow: pulses per read-back
MF_GLOBAL_EVERY = 32     # maxflow: pulses between two global relabels

LADDER_DEGS = (4095, 4096, 4097, 8191, 8192, 8193)   # 0, 1, 2, 2, 2 and 3 chunks
LADDER_CHUNKS = (0, 1, 2, 2, 2, 3)
LEAF0 = 256
LADDER_N = LEAF0 + 8193 + 37                          # 8486: 38 vertices in the last word
LADDER_HUBS = (0, 63, 64, 127, 200, LADDER_N - 1)     # lane 0 and lane 63 of a word, twice; mid-word; the partial last word
WORD_SIZES = (63, 64, 65, 127, 128, 129)


def _finish(n, rows, cols):
    key = np.unique(np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64))
    return key // n, key % n


unique_pairs = _finish


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def sym(rows, cols):
    """both directions of every pair"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


def degrees(n, rows):
    return np.bincount(np.asarray(rows, dtype=np.int64), minlength=n)


def bitmap(act):
    """bool[n] -> the n-bit LSB-first u64 words the procedures take"""
    n = len(act)
    bits = np.zeros((n + 63) // 64 * 64, dtype=bool)
    bits[:n] = act
    return np.packbits(bits, bitorder="little").view(U64).copy()


def dirty_bitmap(act):
    """the same words with every bit at and past n set in the last one (equal to the clean words when n % 64 == 0)"""
    n = len(act)
    bits = bitmap(act)
    if n % 64:
        bits[-1] |= U64(~((1 << (n % 64)) - 1) & 0xFFFFFFFFFFFFFFFF)
    return bits


# ---- the hub ladder ----------------------------------------------------------------------------------------------------

def _ladder_out(degs, hubs, n, short=True, flip=False):
    """hub k -> the first (flip: the last) degs[k] leaves; every 97th leaf -> one of the hubs that point at it, in turn;
    1 -> 2 -> 3"""
    rows, cols = [], []
    top = max(degs)
    for d, h in zip(degs, hubs):
        rows.append(np.full(d, h, dtype=np.int64))
        cols.append(LEAF0 + np.arange(d, dtype=np.int64) + (top - d if flip else 0))
    for j in range(0, top, 97):
        mine = [h for d, h in zip(degs, hubs) if (j >= top - d if flip else j < d)]
        rows.append(np.array([LEAF0 + j], dtype=np.int64))
        cols.append(np.array([mine[(j // 97) % len(mine)]], dtype=np.int64))
    if short:
        rows.append(np.array([1, 2], dtype=np.int64))
        cols.append(np.array([2, 3], dtype=np.int64))
    return _finish(n, np.concatenate(rows), np.concatenate(cols))


@lru_cache(maxsize=None)
def hub_ladder(direction, flip=False):
    """(n, rows, cols): one graph with rows of LADDER_DEGS entries at LADDER_HUBS, over one overlapping range of leaves
    (LEAF0 .. LEAF0 + 8192; 36 vertices without entries and the last hub follow).  A leaf that points back points at a hub whose
    row holds it, so the symmetric form's hub rows have LADDER_DEGS entries too, and every search ends after a few levels.
    direction: "out" = the hub rows are rows of A, "in" = the transpose (rows of A'), "sym" = both directions.
    flip: hub k points at the LAST LADDER_DEGS[k] leaves.  The leaves every hub shares — the ones that take vertex 0's label in
    label propagation, and the lightest or first entries of a row — then sit in the last chunks of the long rows, not in
    their first: a fold that loses a later chunk, or that does not add a label's votes up across chunks, shows."""
    n = LADDER_N
    rows, cols = _ladder_out(LADDER_DEGS, LADDER_HUBS, n, flip=flip)
    if direction == "in":
        rows, cols = _finish(n, cols, rows)
    elif direction == "sym":
        rows, cols = _finish(n, *sym(rows, cols))
    else:
        assert direction == "out"
    return (n,) + _frozen(rows, cols)


@lru_cache(maxsize=None)
def ladder_masks(n=LADDER_N, hubs=LADDER_HUBS):
    """[(name, active bool[n], clean bitmap, dirty bitmap)]: everything on; the 4096 hub, the 8193 hub and every third leaf off;
    only the hubs and the leaves with an id below 4097 on (every hub row partially masked, the last chunk of the 8193 row — and
    most of the chunk before it — inactive)."""
    ids = np.arange(n)
    leaf = (ids >= LEAF0) & (ids < LEAF0 + max(LADDER_DEGS))
    all_on = np.ones(n, dtype=bool)
    thirds = all_on.copy()
    thirds[[hubs[1], hubs[5]]] = False
    thirds[leaf & ((ids - LEAF0) % 3 == 0)] = False
    few = np.zeros(n, dtype=bool)
    few[list(hubs)] = True
    few[leaf & (ids < 4097)] = True
    out = []
    for name, act in (("all", all_on), ("thirds-off", thirds), ("low-leaves", few)):
        out.append((name,) + _frozen(act, bitmap(act), dirty_bitmap(act)))
    return out


def pair_weights(n, rows, cols, kind):
    """float64 weights that are a function of the unordered pair {row, col}: "distinct" = a bijection of lo * n + hi on 27 bits
    (+ 1: positive integers, sums exact), "equal" = 4.0 everywhere."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if kind == "equal":
        return np.full(len(rows), 4.0)
    assert kind == "distinct" and n * n < (1 << 27)
    key = np.minimum(rows, cols) * n + np.maximum(rows, cols)
    return ((key * 0x9E3779B1) % (1 << 27) + 1).astype(np.float64)


@lru_cache(maxsize=None)
def ladder_flow(degs=LADDER_DEGS, mirror=False):
    """(n, rows, cols, caps, src, sink, hubs): the ladder's hub rows as a flow network with dyadic capacities.  The residual
    network stores every pair in both rows, so a hub's row there is its leaves AND the source: hub k points at degs[k] - 1
    leaves and the source feeds it — degs[k] pairs.  The sink is fed by every leaf (a leaf whose id is a multiple of 5 by a
    zero capacity: a dead end that hands its excess back).  mirror = every arc reversed, source and sink swapped: the hubs
    gather.  `degs` may be a part of LADDER_DEGS; the hubs keep the ids LADDER_HUBS gives those degrees."""
    hubs = tuple(LADDER_HUBS[LADDER_DEGS.index(d)] for d in degs)
    n = LADDER_N + 2
    src, sink = LADDER_N, LADDER_N + 1
    rows, cols = _ladder_out(tuple(d - 1 for d in degs), hubs, n, short=False)
    key = rows * n + cols
    caps = np.where(rows >= LEAF0, 1 + key % 4, 1 + key % 8).astype(np.float64) / 4    # leaf -> hub, hub -> leaf
    leaves = LEAF0 + np.arange(max(degs) - 1, dtype=np.int64)
    hub_total = np.array([caps[rows == h].sum() for h in hubs])
    feed = np.where(np.arange(len(hubs)) % 2 == 0, hub_total + 8.0, np.floor(hub_total / 3))   # not / is the bottleneck
    rows = np.concatenate([rows, np.full(len(hubs), src), leaves])
    cols = np.concatenate([cols, np.array(hubs, dtype=np.int64), np.full(len(leaves), sink)])
    caps = np.concatenate([caps, feed, (leaves % 5).astype(np.float64) / 4])
    if mirror:
        rows, cols, src, sink = cols, rows, sink, src
    order = np.lexsort((cols, rows))
    return (n,) + _frozen(rows[order], cols[order], caps[order]) + (src, sink, hubs)


def shuffled(rows, cols, *more, seed=7):
    """the same entries in another order (a COO the builder has to sort)"""
    p = np.random.default_rng(seed).permutation(len(rows))
    return tuple(np.asarray(x)[p] for x in (rows, cols) + more)


# ---- word edges --------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def word_graphs():
    """{n: (rows, cols, masks)} for n at both sides of one and of two 64-row words: the ring i -> i + 1 plus the chords
    i -> (7 i + 3) mod n; masks = [(name, active, clean bitmap, dirty bitmap)] with every fifth vertex off and the last vertex
    on, then off."""
    out = {}
    for n in WORD_SIZES:
        i = np.arange(n, dtype=np.int64)
        rows, cols = _finish(n, np.concatenate([i, i]), np.concatenate([(i + 1) % n, (7 * i + 3) % n]))
        masks = []
        for name, last in (("last-on", True), ("last-off", False)):
            act = i % 5 != 2
            act[n - 1] = last
            masks.append((name,) + _frozen(act, bitmap(act), dirty_bitmap(act)))
        out[n] = _frozen(rows, cols) + (masks,)
    return out


# ---- batch edges -------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def batch_paths(B=BATCH):
    """{L: {kind: (n, rows, cols)}} for L = 1 .. 2 B + 1, the smallest graph on which a procedure takes L iterations:
    "directed" the path 0 -> 1 -> ... -> L (harmonic: L iterations change a sketch; sssp: the tight tree is L deep);
    "forest"   the path of 2^L + 1 vertices in id order, both directions (a chain 2^L deep halves L times under pointer jumping);
    "flood"    the symmetric path of L vertices with a self-loop on each (cdlp: label[v] = max(0, v - t), the L-th iteration is
               the first that changes nothing);
    "swap"     one symmetric edge (cdlp: its two labels swap for ever, every itermax is reached)."""
    out = {}
    for L in range(1, 2 * B + 2):
        i = np.arange(L, dtype=np.int64)
        k = np.arange(2 ** L, dtype=np.int64)
        j = np.arange(L - 1, dtype=np.int64)
        out[L] = {"directed": (L + 1,) + _frozen(i, i + 1),
                  "forest": (2 ** L + 1,) + _frozen(*_finish(2 ** L + 1, *sym(k, k + 1))),
                  "flood": (L,) + _frozen(*_finish(L, np.concatenate([j, j + 1, i]), np.concatenate([j + 1, j, i]))),
                  "swap": (2,) + _frozen(np.array([0, 1], dtype=np.int64), np.array([1, 0], dtype=np.int64))}
    return out


def pointer_jumps(parent):
    """how many times parent = parent[parent] changes something"""
    parent = np.asarray(parent, dtype=np.int64)
    jumps = 0
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            return jumps
        parent, jumps = nxt, jumps + 1


def bottleneck_path(n):
    """(rows, cols, caps) of the path 0 -> ... -> n - 1 with capacity 10 and one arc of 3.25 in the middle"""
    caps = np.full(n - 1, 10.0)
    caps[(n - 1) // 2] = 3.25
    return np.arange(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64), caps
