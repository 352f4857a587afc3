"""Inputs for fgpu_expand_edges (csrc/expand_edges.hip) and fgpu_expand_trails (csrc/expand_trails.hip) that sit on the sizes at
which their scans and binary searches switch, and a plain reference for both.  Numpy and Python only: no GPU, no ctypes.

The reference (`trail_rows`, `edge_rows`) states the rules of oracle.model.var_len_expand and oracle.model.expand_row — per type
the outgoing half then the incoming half, ascending by other node and then id; a LIFO stack, a frame's emissions before any deeper
frame's; an edge id at most once on a trail; CondTraverse's pairs ascending, per pair the types in scan order — over an index that
is built once per tensor (node -> its outgoing and incoming (other, ids) lists, from Tensor.structure() and Tensor.get), where
oracle.model.node_relationships sorts the whole structure on every call.  It shares nothing with tests/trails_check.py, which
restates the device's scan rule.  tests/test_expand_cases_cpu.py holds it against the model and proves what every builder below
claims; tests/test_gpu_expand_cases.py runs the families on the device.

The families, each the smallest shape at which the named code can still go wrong:
  A  layer_merge      the two-layer adjacency slot of et_gather_kernel: m and dp runs of 0 .. 130 entries merged by rank
  B  many_types       64 types of which three hold entries: stretches of >= 64 empty segments / count-0 items in a wordrow word
  C  irregular_tree   et_sum / et_base / et_root over levels of 9000 and 18 000 frames with childless frames at the tile edges
  D  parallel_*       used edge ids inside multi-edge id lists of 63 .. 129 ids
  E  budget_tree      max_items against the `held` value after every single depth
  F  sort_*           expand_edges' one-key / two-sort decision and the staged sort's level classes and block size
  G  word_edge_graph  label bitmaps whose deciding bit is in the last, partial word
"""
import numpy as np

from oracle.model import MULTI_EDGE, Graph, Tensor

# ---- the kernel constants the cases are built around (tests/test_expand_cases_cpu.py reads them back from the sources) ------
WORD = 64                      # entries per wordrow word (bulk.hpp: wordrow_kernel, `w << 6`; entry_vec, `p >> 6`)
BLOCK = 256                    # lanes per block of every kernel of the two files (__launch_bounds__(256))
SCAN_TILE = 4096               # items per block of scan_u32 / scan_u32_to_u64 (prims.hip: SCAN_THREADS * SCAN_SUBTILES)
KP_EB = 2048                   # entries per block of sort_pairs_by_key_staged (transpose.hip)
KP_BITS = 9                    # bits a level of that sort; kp_widths: kb = ceil(log2(keys)), ceil(kb / 9) levels, 3 from kb = 17
KP_THREE_LEVELS_KB = 17
ONE_KEY_LIMIT = 1 << 22        # expand_edges.hip: one key (row * P + pass) * n + other while nrp * n <= this, else two sorts
EE_MAX_TYPES = 64              # edge_layers.hpp; the packed type word keeps the position in `& 63`, bit 31 = "id from the table"
TRAILS_MAX_DEPTH = 64          # fgpu.h: FGPU_TRAILS_MAX_DEPTH

DIRECTIONS = ("out", "in", "both")


def kp_levels(nkeys):
    """the level count kp_widths (sort_plan.hpp) gives a key space of nkeys"""
    kb = 1
    while kb < 32 and (1 << kb) < nkeys:
        kb += 1
    L = max(1, (kb + KP_BITS - 1) // KP_BITS)
    if kb >= KP_THREE_LEVELS_KB and L < 3:
        L = 3
    return min(L, kb)


# ---- the reference -------------------------------------------------------------------------------------------------------
class TensorIndex:
    """out[v] / inn[v]: [(other, ids)] ascending by other over the effective structure, ids ascending (Tensor.get)"""

    def __init__(self, T):
        self.out, self.inn = {}, {}
        for (s, d) in T.structure():
            ids = T.get(s, d)
            self.out.setdefault(s, []).append((d, ids))
            self.inn.setdefault(d, []).append((s, ids))
        for rows in (self.out, self.inn):
            for v in rows:
                rows[v].sort(key=lambda x: x[0])
        self.outd = {v: dict(r) for v, r in self.out.items()}


_INDEX = {}


def index_of(T):
    if id(T) not in _INDEX:
        _INDEX[id(T)] = (T, TensorIndex(T))           # (the tensor is kept: its id stays its own)
    return _INDEX[id(T)][1]


def scan_of(g, types):
    """type names -> tensor positions, in the order given; () = every tensor"""
    return [g.type_ids[t] for t in types] if types else list(range(len(g.tensors)))


def labelled(g, labels):
    """the nodes carrying every label of `labels`, or None for no label (= no bitmap)"""
    if not labels:
        return None
    lids = [g.label_ids[l] for l in labels]
    return frozenset(v for v in range(g.n) if all((v, l) in g.node_labels for l in lids))


def adjacency(g, node, scan, direction):
    """[(neighbour, ids)] of a frame at `node`: per type the outgoing half, then the incoming half (without the self-loop when the
    outgoing half was walked), each ascending by other node, the ids of a pair ascending"""
    out = []
    for t in scan:
        ix = index_of(g.tensors[t])
        if direction != "in":
            out += ix.out.get(node, ())
        if direction != "out":
            out += [(o, ids) for (o, ids) in ix.inn.get(node, ()) if not (direction == "both" and o == node)]
    return out


def trail_rows(g, start, dest=None, types=(), lo=1, hi=None, direction="out", bitmap_nodes=None, counters=None,
               _siblings="lifo"):
    """CondVarLenTraverse over one row: [(from, to, path)] in the reference's emission order, path = [node, edge, node, ...] in
    pattern order (reversed when direction == "in").  counters (a dict) receives frames / used / levels / multi: what stats[0],
    [2], [4] and [6] of the device call count.  _siblings="forward" is the deliberately wrong order of the discrimination test."""
    scan = scan_of(g, types)
    rev = direction == "in"
    ok = lambda v: (dest is None or dest == v) and (bitmap_nodes is None or v in bitmap_nodes)
    rows = []

    def emit(other, walk):
        rows.append((other, start, walk[::-1]) if rev else (start, other, walk))     # (a walk is never changed once built)

    if lo == 0 and ok(start):
        emit(start, [start])
    frames = used_drops = levels = multi = 0
    adj = {}
    stack = [(start, [start], (), 0)]
    runs = hi is None or (hi >= 1 and lo <= hi)
    while stack and runs:
        node, walk, used, depth = stack.pop()
        hop = depth + 1
        frames += 1
        levels = max(levels, hop)
        if node not in adj:
            items = adjacency(g, node, scan, direction)
            adj[node] = ([(e, o) for (o, ids) in items for e in ids], sum(1 for (_, ids) in items if len(ids) > 1))
        multi += adj[node][1]
        children = []
        for (e, nb) in adj[node][0]:
            if e in used:
                used_drops += 1
                continue
            nwalk = walk + [e, nb]
            if hop >= lo and ok(nb):
                emit(nb, nwalk)
            if hi is None or hop < hi:
                children.append((nb, nwalk, used + (e,), hop))
        stack += children if _siblings == "lifo" else children[::-1]
    if counters is not None:
        for k_, v in (("frames", frames), ("used", used_drops), ("multi", multi)):
            counters[k_] = counters.get(k_, 0) + v
        counters["levels"] = max(counters.get("levels", 0), levels)
    return rows


def edge_rows(g, frm, to, types=(), transposed=False, bidirectional=False, first_only=False, from_nodes=None, to_nodes=None,
              with_pass=False, _types="scan"):
    """CondTraverse's per-row path for one row: [(from, to, id)] ([(from, to, id, pass, type position)] with_pass) in emission order.  The
    forward pass walks the row of the matrix source (ascending column, cut to the destination when bound), or with only the
    destination bound that row of the transposed structure; the bidirectional pass swaps the endpoints and drops self-loops.
    Per pair the types in scan order, ids ascending; first_only keeps the first.  from_nodes / to_nodes: node sets (label
    bitmaps) the oriented endpoints must lie in.  _types="descending" is the wrong order of the discrimination test."""
    scan = scan_of(g, types)
    ixs = [index_of(g.tensors[t]) for t in scan]
    out = []
    if frm is None and to is None:
        return out

    def others(rows_name, v):
        return sorted(set(o for ix in ixs for (o, _) in getattr(ix, rows_name).get(v, ())))

    def one_pass(msrc, mdst, against, drop_loops, p):
        if msrc is not None:
            pairs = [(msrc, d) for d in others("out", msrc) if mdst is None or d == mdst]
        else:
            pairs = [(s, mdst) for s in others("inn", mdst)]
        for (s, d) in pairs:
            if drop_loops and s == d:
                continue
            fn, tn = (d, s) if against else (s, d)
            if (from_nodes is not None and fn not in from_nodes) or (to_nodes is not None and tn not in to_nodes):
                continue
            order = list(enumerate(ixs)) if _types == "scan" else list(enumerate(ixs))[::-1]
            ids = [(e, pos) for pos, ix in order for e in ix.outd.get(s, {}).get(d, ())]
            for e, pos in ids[:1] if first_only else ids:
                out.append((fn, tn, e, p, pos) if with_pass else (fn, tn, e))

    fwd = (to, frm) if transposed else (frm, to)
    one_pass(fwd[0], fwd[1], transposed, False, 0)
    if bidirectional:
        one_pass(fwd[1], fwd[0], not transposed, True, 1)
    return out


def edge_counters(want):
    """what the (N, 6) rows of edge_columns pin of the device's counters: (pair, type) items that emitted, multi-edge pairs among
    them, the longest list"""
    if not len(want):
        return {"items": 0, "multi": 0, "longest": 0}
    key = want[:, [0, 4, 1, 2, 5]]
    first = np.concatenate([[True], (key[1:] != key[:-1]).any(axis=1)])
    sizes = np.diff(np.concatenate([np.nonzero(first)[0], [len(want)]]))
    return {"items": int(first.sum()), "multi": int((sizes > 1).sum()), "longest": int(sizes.max())}


def trail_columns(g, starts, dests=None, memo=None, types=(), lo=1, hi=None, direction="out", bitmap_nodes=None):
    """(row, from, to, hops, path_off, path_node, path_edge) as int64 arrays for a batch, and the counters of the whole batch.
    The walk of a start does not depend on lo, dest or the bitmap — they only decide which children emit — so trail_rows runs once
    per distinct start, unfiltered from 0 hops, and the rows of a (start, dest) are those of its emissions that pass.  memo (a dict
    the caller keeps per (graph, types, hi, direction)) carries the walks and the filtered columns from batch to batch."""
    memo = {} if memo is None else memo
    cols, counters = [[] for _ in range(6)], {"frames": 0, "used": 0, "multi": 0, "levels": 0}
    runs = hi is None or (hi >= 1 and lo <= hi)
    i64 = lambda xs: np.array(xs, dtype=np.int64)
    for i, s in enumerate(starts):
        s, d = int(s), None if dests is None else dests[i]
        key = (s, d, lo, bitmap_nodes)
        if key not in memo:
            if runs:
                if ("walk", s) not in memo:
                    c = {}
                    memo[("walk", s)] = (trail_rows(g, s, None, types, 0, hi, direction, counters=c), c)
                walk, c = memo[("walk", s)]
                other = 0 if direction == "in" else 1
                rows = [r for r in walk if len(r[2]) // 2 >= lo and (d is None or r[other] == d) and
                        (bitmap_nodes is None or r[other] in bitmap_nodes)]
            else:
                c = {}
                rows = trail_rows(g, s, d, types, lo, hi, direction, bitmap_nodes, counters=c)
            memo[key] = (i64([r[0] for r in rows]), i64([r[1] for r in rows]), i64([len(r[2]) // 2 for r in rows]),
                         i64([v for r in rows for v in r[2][0::2]]), i64([e for r in rows for e in r[2][1::2]]), c)
        f, t, h, pn, pe, c = memo[key]
        for col, a in zip(cols, (np.full(len(f), i, dtype=np.int64), f, t, h, pn, pe)):
            col.append(a)
        for name in ("frames", "used", "multi"):
            counters[name] += c[name]
        counters["levels"] = max(counters["levels"], c["levels"])
    row, f, t, h, pn, pe = [np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols]
    off = np.concatenate([[0], np.cumsum(h)]).astype(np.int64) if len(h) else np.zeros(0, dtype=np.int64)
    return (row, f, t, h, off, pn, pe), counters


def edge_columns(g, froms, tos, memo=None, **kw):
    """(N, 6) uint64: row, from, to, id, pass, type position for a batch, edge_rows once per distinct (from, to)"""
    memo = {} if memo is None else memo
    out = []
    for i, key in enumerate(zip(froms, tos)):
        if key not in memo:
            memo[key] = np.array(edge_rows(g, key[0], key[1], with_pass=True, **kw), dtype=np.uint64).reshape(-1, 5)
        a = memo[key]
        out.append(np.concatenate([np.full((len(a), 1), i, dtype=np.uint64), a], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 6), dtype=np.uint64)


# ---- building graphs -----------------------------------------------------------------------------------------------------
def graph_of_tensors(n, tensors, labels=None):
    """tensors: [(type name, m, dp, dm, me)]; labels: {name: nodes}"""
    g = Graph(n)
    for name, m, dp, dm, me in tensors:
        g.add_type(name)
        g.tensors[g.type_ids[name]] = Tensor(n, n, m=m, dp=dp, dm=dm, me=me)
    g.adjacency.m = set().union(*[t.structure() for t in g.tensors]) if g.tensors else set()
    for name, nodes in (labels or {}).items():
        lid = g.add_label(name)
        g.node_labels |= {(int(v), lid) for v in nodes}
    return g


class _Ids:
    def __init__(self, first):
        self.next = first

    def __call__(self, k=1):
        self.next += k
        return list(range(self.next - k, self.next))


# ---- A: the two-layer adjacency slot -------------------------------------------------------------------------------------
RUNS = ((63, 1), (64, 64), (65, 63), (1, 65), (130, 130), (0, 70), (70, 0))     # (m run, dp run) of a hub
PATTERNS = ("interleave", "dp_below", "dp_above", "identical")
A_N = 700
A_OPENERS = (56, 57, 58, 59)   # roots with 0, 1, 2 and 3 entries in each direction
A_LEAF0 = 60                   # nodes 60 .. 699 are the hubs' neighbours


def hub_neighbours(a, b, pattern, base):
    """(m neighbours, dp neighbours) of a hub, each ascending"""
    if pattern == "interleave":
        return [base + 2 * i for i in range(a)], [base + 2 * j + 1 for j in range(b)]
    if pattern == "dp_below":
        return [base + b + i for i in range(a)], [base + j for j in range(b)]
    if pattern == "dp_above":
        return [base + i for i in range(a)], [base + a + j for j in range(b)]
    return [base + i for i in range(a)], [base + j for j in range(b)]      # identical: min(a, b) shared, shadowed pairs


def layer_merge(runs=RUNS, n=A_N, leaf0=A_LEAF0, spread=370):
    """One type with unfolded deltas.  Hub h (one per (run lengths, pattern), node h) has an m run and a dp run of the given
    lengths in its OUT row; its mirror (node h + H) has the same runs in its IN row, that is in mt_m / mt_dp when the transposed
    layers are passed as layers.  Every 7th m entry (i % 7 == 3) is tombstoned in dm — under `identical` that pair is also in dp,
    tombstoned and re-added; entry 1 of m and entry 0 of dp are multi-edge pairs where the pattern leaves them live.  The leaves
    form one cycle leaf -> next(leaf), so every level-1 frame has a second hop in each direction.  Returns (graph, hubs), hubs =
    [(node, mirror, a, b, pattern, m neighbours, dp neighbours)]."""
    eid = _Ids(1000)
    m, dp, dm, me = {}, {}, set(), {}
    hubs = []
    H = len(runs) * len(PATTERNS)
    assert 2 * H <= A_OPENERS[0] or n != A_N
    nleaf = n - leaf0
    for r, (a, b) in enumerate(runs):
        for q, pattern in enumerate(PATTERNS):
            h = r * len(PATTERNS) + q
            mn, dn = hub_neighbours(a, b, pattern, leaf0 + (h * 17) % spread)
            assert not mn + dn or max(mn + dn) < n
            hubs.append((h, h + H, a, b, pattern, mn, dn))
            for pair in (lambda x: (h, x), lambda x: (x, h + H)):
                for i, x in enumerate(mn):
                    p = pair(x)
                    if i == 1 and x not in dn:
                        m[p], me[p] = MULTI_EDGE, eid(3)
                    else:
                        m[p] = eid()[0]
                    if i % 7 == 3:
                        dm.add(p)
                for j, x in enumerate(dn):
                    p = pair(x)
                    if j == 0:
                        dp[p], me[p] = MULTI_EDGE, eid(2)
                    else:
                        dp[p] = eid()[0]
    step = 13
    assert np.gcd(step, nleaf) == 1
    for v in range(nleaf):
        m[(leaf0 + v, leaf0 + (v * step + 5) % nleaf)] = eid()[0]
    for j, root in enumerate(A_OPENERS if n == A_N else ()):
        for i in range(j):
            m[(root, leaf0 + i)] = eid()[0]
            m[(leaf0 + i, root)] = eid()[0]
    return graph_of_tensors(n, [("T", m, dp, dm, me)]), hubs


def layer_merge_small():
    """the same structure with runs of at most 5: for the cross-checks against the model"""
    return layer_merge(runs=((3, 1), (4, 4), (5, 3), (1, 5), (0, 4), (4, 0)), n=160, leaf0=60, spread=80)


def merge_edge_rows(hubs):
    """(froms, tos) for expand_edges: (hub, None), (None, mirror), the two the other way round, and (hub, x) with x in m only,
    in dp only, shadowed and tombstoned where the hub has such a neighbour"""
    froms, tos = [], []
    for (h, mir, a, b, pattern, mn, dn) in hubs:
        dead = [x for i, x in enumerate(mn) if i % 7 == 3 and x not in dn]
        kinds = ([x for i, x in enumerate(mn) if x not in dn and i % 7 != 3][:1], [x for x in dn if x not in mn][:1],
                 [x for x in mn if x in dn][:1], dead[:1])
        for f, t in [(h, None), (None, mir), (mir, None), (None, h)] + [(h, k[0]) for k in kinds if k] + [(k[0], mir) for k in kinds if k]:
            froms.append(f)
            tos.append(t)
    return froms, tos


# ---- B: many types, empty stretches ----------------------------------------------------------------------------------------
B_TYPES = tuple("T%02d" % t for t in range(EE_MAX_TYPES))
B_HELD = (0, 31, 63)           # the type positions that hold entries
B_N = 96
B_ROWS = 300
B_EVERY = 50                   # every 50th row of the batch starts at a populated node


def many_types(ntypes=EE_MAX_TYPES, held=B_HELD, n=B_N, nodes=6):
    """ntypes types, only those at `held` with entries.  Populated node p (p < nodes): first held type (p, 40), (p, 41); the middle
    one m (p, 41) and dp (p, 42) — the one dp layer, so a frame has ntypes x 2 x 2 segments under bidirectional; the last one
    (p, 40) again, (p, 43) as a multi-edge pair, and the in-edge (44, p).  Nodes 40 and 43 lead on to node (p + 1) % nodes."""
    eid = _Ids(5000)
    tensors = []
    for t in range(ntypes):
        m, dp, me = {}, {}, {}
        for p in range(nodes):
            if t == held[0]:
                m[(p, 40)], m[(p, 41)] = eid()[0], eid()[0]
                m[(40, (p + 1) % nodes)] = eid()[0]
            elif t == held[1]:
                m[(p, 41)], dp[(p, 42)] = eid()[0], eid()[0]
            elif t == held[2]:
                m[(p, 40)] = eid()[0]
                m[(p, 43)], me[(p, 43)] = MULTI_EDGE, eid(3)
                m[(44, p)] = eid()[0]
                m[(43, (p + 1) % nodes)] = eid()[0]
        tensors.append(("T%02d" % t, m, dp, set(), me))
    return graph_of_tensors(n, tensors)


def many_types_rows(k=B_ROWS, every=B_EVERY, nodes=6):
    """k start nodes: every `every`-th one populated (0, 1, ...), the rest among the isolated nodes 60 .. 69"""
    return [(i // every) % nodes if i % every == 0 else 60 + i % 10 for i in range(k)]


TOMB_RUN = 130


def tombstones(run=TOMB_RUN, n=300):
    """node 0's m row: `run` tombstoned entries, then one live one; node 1's IN row the same (pairs (x, 1)); the live neighbour
    leads on to node 2 and is reached from node 3"""
    m, dm = {}, set()
    eid = _Ids(100)
    for i in range(run + 1):
        m[(0, 100 + i)] = eid()[0]
        m[(100 + i, 1)] = eid()[0]
        if i < run:
            dm |= {(0, 100 + i), (100 + i, 1)}
    m[(100 + run, 2)] = eid()[0]
    m[(3, 100 + run)] = eid()[0]
    return graph_of_tensors(n, [("T", m, {}, dm, {})])


# ---- C: an irregular tree across scan tiles ----------------------------------------------------------------------------------
C_CHILDREN = 9000
C_EDGE_POSITIONS = (0, 255, 256, 4095, 4096)       # ... and the last of the level


def _labels(count, mod):
    """position -> label: the identity, but for the swaps that put a label with label % mod == 0 at positions 0, 255, 256, 4095, 4096
    and count - 1 (where they lie inside the level)"""
    lab = list(range(count))
    for p in C_EDGE_POSITIONS + (count - 1,):
        if p < count and lab[p] % mod:
            q = next(x for x in range(p + 1, count) if lab[x] % mod == 0 and x not in C_EDGE_POSITIONS) if p != count - 1 else \
                next(x for x in range(p - 1, -1, -1) if lab[x] % mod == 0 and x not in C_EDGE_POSITIONS)
            lab[p], lab[q] = lab[q], lab[p]
    return lab


def irregular_tree(children=C_CHILDREN):
    """Root 0 with `children` children; the child labelled j has j % 5 children, the grandchild labelled g has g % 3.  Nodes are
    numbered level by level in adjacency order, so a frame's position in its level is its node id minus the level's first id.
    Returns (graph, level sizes, per-level child counts by position)."""
    lab1 = _labels(children, 5)
    c1 = [j % 5 for j in lab1]
    n2 = sum(c1)
    lab2 = _labels(n2, 3)
    c2 = [x % 3 for x in lab2]
    n3 = sum(c2)
    first = (0, 1, 1 + children, 1 + children + n2)
    m = {(0, 1 + p): 10 ** 6 + p for p in range(children)}
    nxt = first[2]
    for p, c in enumerate(c1):
        for _ in range(c):
            m[(first[1] + p, nxt)] = 2 * 10 ** 6 + nxt
            nxt += 1
    for p, c in enumerate(c2):
        for _ in range(c):
            m[(first[2] + p, nxt)] = 2 * 10 ** 6 + nxt
            nxt += 1
    n = 1 + children + n2 + n3
    assert nxt == n
    g = graph_of_tensors(n, [("T", m, {}, set(), {})], labels={"K": [v for v in range(n) if v % 3 == 1]})
    return g, (1, children, n2, n3), (c1, c2)


MANY_ROOTS = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)


def many_roots_graph():
    """12 nodes in a ring with chords and one multi-edge pair; the even nodes carry the label K"""
    m = {(v, (v + 1) % 12): 100 + v for v in range(12)}
    m.update({(v, (v + 5) % 12): 200 + v for v in range(0, 12, 3)})
    m[(1, 2)] = MULTI_EDGE
    return graph_of_tensors(12, [("T", m, {}, set(), {(1, 2): [300, 301]})], labels={"K": range(0, 12, 2)})


def many_roots(k):
    """(starts, dests): every fifth root (i % 5 == 4) starts at an odd node, which the bitmap K filters out; every third root's
    dest is its own start, so with lo = 0 its 0-hop row survives and little else"""
    starts = [(2 * (i % 6) + 1) % 12 if i % 5 == 4 else 2 * (i % 6) for i in range(k)]
    return starts, [s if i % 3 == 0 else None for i, s in enumerate(starts)]


# ---- D: used edges inside id lists -----------------------------------------------------------------------------------------
def parallel_pair(k=4):
    """two nodes joined by k parallel edges 0 -> 1"""
    return graph_of_tensors(2, [("T", {(0, 1): MULTI_EDGE}, {}, set(), {(0, 1): list(range(10, 10 + k))})])


def trails_between_two(k):
    """trails from one end over k parallel edges walked both ways: k + k (k - 1) + ... + k!"""
    total, term = 0, 1
    for i in range(k):
        term *= k - i
        total += term
    return total


def parallel_ring(side=3, per=3):
    """a ring of `side` nodes, `per` parallel edges v -> v + 1 on each side"""
    m = {(v, (v + 1) % side): MULTI_EDGE for v in range(side)}
    me = {(v, (v + 1) % side): list(range(100 * (v + 1), 100 * (v + 1) + per)) for v in range(side)}
    return graph_of_tensors(side, [("T", m, {}, set(), me)])


RING_TRAILS = 3 + 9 + 27 + 27 * 2      # per start on parallel_ring(3, 3), one way, hi = 4: the 4th hop is back on the first side, 2 ids left
LISTS = (63, 64, 65, 129)


def id_lists(lists=LISTS):
    """root 0 -> node 1 + i over lists[i] parallel edges.  Walked both ways with hi = 2, a frame at node 1 + i (reached over one id
    of its list) meets that list again in its incoming half, the used id inside it: lists[i] - 1 emissions per frame."""
    m = {(0, 1 + i): MULTI_EDGE for i in range(len(lists))}
    me, eid = {}, _Ids(1000)
    for i, L in enumerate(lists):
        me[(0, 1 + i)] = eid(L)
    return graph_of_tensors(1 + len(lists), [("T", m, {}, set(), me)])


# ---- E: the budget per level -----------------------------------------------------------------------------------------------
E_FAN, E_DEPTH = 3, 4


def budget_tree(fan=E_FAN, depth=E_DEPTH):
    """the complete `fan`-ary tree of `depth` levels below the root, node ids level by level"""
    m, nxt, level = {}, 1, [0]
    for _ in range(depth):
        below = []
        for v in level:
            for _ in range(fan):
                m[(v, nxt)] = 500 + nxt
                below.append(nxt)
                nxt += 1
        level = below
    return graph_of_tensors(nxt, [("T", m, {}, set(), {})])


def held_after(d, fan=E_FAN, hi=E_DEPTH, k=1):
    """frames + emissions held after depth d was expanded, lo = 1: the roots, and per expanded depth i its fan^(i+1) emissions and,
    while hop i + 1 < hi, as many new frames"""
    return k + sum(k * fan ** (i + 1) * (2 if i + 1 < hi else 1) for i in range(d + 1))


# ---- F: the sort decision and the key-space classes ------------------------------------------------------------------------
F_TYPES = ("C", "A", "B")      # the scan order of every F case: not ascending


def sort_graph(n, nodes=None, seed=3):
    """three types A, B, C over shared pairs among `nodes` (default: all n): about half of the pairs sit in two or three types, every
    8th entry is a multi-edge pair; type B carries a dp layer (a shadowed pair and a dp-only pair per 16 pairs)"""
    rng = np.random.default_rng(seed)
    nodes = list(range(n)) if nodes is None else nodes
    eid = _Ids(10 ** 6)
    pairs = sorted({(int(nodes[a]), int(nodes[b])) for a, b in rng.integers(0, len(nodes), (3 * len(nodes), 2))})
    tensors = []
    for t, name in enumerate("ABC"):
        m, dp, me = {}, {}, {}
        for j, p in enumerate(pairs):
            if (j + t) % 3 == 0 and j % 2:
                continue                                       # (every pair is in at least two types; the even ones in all three)
            if (j + t) % 8 == 0:
                m[p], me[p] = MULTI_EDGE, eid(2 + j % 3)
            else:
                m[p] = eid()[0]
            if name == "B" and j % 16 == 5:
                dp[p] = eid()[0]
            if name == "B" and j % 16 == 9:
                dp[(p[0], nodes[(j * 7) % len(nodes)])] = eid()[0]
        tensors.append((name, m, dp, set(), me))
    return graph_of_tensors(n, tensors)


def key_space_cases():
    """[(name, n, k, bidirectional, sort path, levels of the staged sort)]: k x P x n on both sides of every class boundary.  The
    level count changes where ceil(log2(keys)) does: 2^9 -> 2^9 + n (1 -> 2 levels), 2^16 -> 2^16 + n (2 -> 3: kb = 17), so the
    two cases around 2^17 are both three-level; 2^22 -> 2^22 + n is the switch to two sorts (keys = max(n, k P) there)."""
    out = []
    for name, n, k, bidir in (("2^9", 64, 8, False), ("2^9+n", 64, 9, False), ("2^16", 1024, 32, True), ("2^16+n", 1024, 65, False),
                              ("2^17-n", 1024, 127, False), ("2^17", 1024, 64, True), ("2^22", 1024, 4096, False),
                              ("2^22+n", 1024, 4097, False)):
        keys = k * (2 if bidir else 1) * n
        path = 1 if keys <= ONE_KEY_LIMIT else 2
        out.append((name, n, k, bidir, path, kp_levels(keys if path == 1 else max(n, k * (2 if bidir else 1)))))
    return out


def key_space_rows(n, k):
    """k bound sources cycling through every node, no two neighbours in the batch alike"""
    return [(i * 37 + i // n) % n for i in range(k)]


STABLE_N = 1 << 20
STABLE_ENT = (2047, 2048, 2049, 4097, 70000)
STABLE_HUB = 777


def stable_graph(n_ent, n=STABLE_N):
    """One hub row of n_ent stored entries over the three types: n_ent // 3 pairs held by A, B and C alike, and n_ent % 3 more pairs in
    A only.  Every 10th pair is multi-edge in B.  Scanned as C, A, B from STABLE_ROWS (the hub among four isolated nodes), the batch's key space
    is 5 n > 2^22 (two sorts), every entry of the second sort has the same key, and only stability keeps the type order."""
    eid = _Ids(10 ** 7)
    d, r = divmod(n_ent, 3)
    others = [1000 + 13 * i for i in range(d + r)]
    assert others[-1] < n
    tensors = []
    for t, name in enumerate("ABC"):
        m, me = {}, {}
        for i, x in enumerate(others):
            if i >= d and t > 0:
                continue                                       # (the extras are in A only)
            p = (STABLE_HUB, x)
            if name == "B" and i % 10 == 0:
                m[p], me[p] = MULTI_EDGE, eid(2)
            else:
                m[p] = eid()[0]
        tensors.append((name, m, {}, set(), me))
    return graph_of_tensors(n, tensors)


STABLE_ROWS = (5, 6, STABLE_HUB, 7, 8)


# ---- G: bitmaps at word edges ----------------------------------------------------------------------------------------------
G_SIZES = (63, 64, 65, 127, 128, 129)


def word_edge_graph(n):
    """a complete digraph (with a self-loop and a multi-edge pair) over the nodes 0, 1, 62, 63, 64, n - 2, n - 1 that exist.  Label
    F: node n - 1 and node 63; label Q: node n - 1, node 64 and node 0 (those below n)."""
    special = sorted({v for v in (0, 1, 62, 63, 64, n - 2, n - 1) if 0 <= v < n})
    eid = _Ids(100)
    m, me = {}, {}
    for a in special:
        for b in special:
            if a != b or a == n - 1:
                m[(a, b)] = eid()[0]
    m[(n - 1, 0)], me[(n - 1, 0)] = MULTI_EDGE, eid(2)
    g = graph_of_tensors(n, [("T", m, {}, set(), me)],
                         labels={"F": [v for v in (n - 1, 63) if v < n], "Q": [v for v in (n - 1, 64, 0) if v < n]})
    return g, special


def dirty_bits(words, n):
    """the bitmap with every bit at and past n set in its last word"""
    out = np.array(words, dtype=np.uint64, copy=True)
    if n % 64:
        out[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
    return out
