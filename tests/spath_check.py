"""Checker for fgpu_shortest_path_batch and Graph.shortest_path (no GPU, no engine import): the contract of include/fgpu.h — the
reference's bfs_shortest_path (runtime/eval.rs:1386-1513) — restated in plain Python.

shortest_path(n, rows, cols, src, dst, max_hops, undirected, prepared=None) -> (path | None, stats8)
    The pattern is the set of entries (rows[k], cols[k]); the forward side reads F = the pattern, the backward side its
    transpose; undirected: both read S = F U F'.  neighbors(v) = the columns of row v, ascending, each once.  Each ball
    starts as its seed at depth 0.  A round: no path when a frontier is empty or df + db >= max_hops (< 0: unbounded); the
    forward side expands iff it has at most as many frontier vertices as the backward side; it walks its frontier in order
    and each row in ascending column order; a vertex outside its own ball is claimed by the first entry that reaches it
    (parent = that row's vertex, depth = the level); a claimed vertex the other ball holds is a meeting candidate, the others
    form the next frontier in walk order; the level runs to its end; the meeting vertex is the candidate of the least other
    depth, the first such.  path = src .. meeting vertex by the forward parents, then on to dst by the backward parents.
    stats8 = [forward levels, backward levels, vertices claimed forward, claimed backward (seeds not counted), entries walked,
    the meeting vertex or 2^64 - 1, meeting candidates of the last level, 0].
prepare(n, rows, cols, undirected) -> the two neighbour tables, for several calls on one pattern.

reference_path(edges, src, dst, types, directed, min_hops, max_hops) -> None | (nodes, edge ids)
    eval_shortest_path over an edge list [(id, type, src, dst), ...]: src / dst None = a Null endpoint (null path); types =
    the pattern's names in order, [] = none named (then the graph's type order: first appearance in `edges`); a named type no
    edge has does not exist; with names of which none exists there is no neighbour stream and so no path.  min_hops 0 with
    src == dst is the one-node path; a path shorter than min_hops is null.  The relationship of a consecutive pair (u, v) is
    the first id of the types in order from u to v, else the first from v to u (tried in the directed case too), else none."""
import numpy as np

NO_MEET = (1 << 64) - 1


def _table(n, rows, cols):
    key = np.unique(np.asarray(rows, dtype=np.int64).ravel() * n + np.asarray(cols, dtype=np.int64).ravel()) if len(rows) else \
        np.zeros(0, dtype=np.int64)
    r, c = key // n, key % n
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    return rp, c


def prepare(n, rows, cols, undirected=False):
    rows, cols = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
    if undirected:
        rows, cols = np.concatenate((rows, cols)), np.concatenate((cols, rows))
        s = _table(n, rows, cols)
        return s, s
    return _table(n, rows, cols), _table(n, cols, rows)


def search(tables, src, dst, max_hops=-1):
    """the rounds over two neighbour tables (forward, backward), each (rowptr, sorted unique columns)"""
    stats = [0, 0, 0, 0, 0, NO_MEET, 0, 0]
    if src == dst:
        return None, stats
    balls = ({src: (src, 0)}, {dst: (dst, 0)})     # vertex -> (parent, depth)
    fronts = [[src], [dst]]
    depth = [0, 0]
    meet = None                                    # (other depth, vertex)
    while meet is None:
        if not fronts[0] or not fronts[1] or (max_hops >= 0 and depth[0] + depth[1] >= max_hops):
            return None, stats
        side = 0 if len(fronts[0]) <= len(fronts[1]) else 1
        rp, ci = tables[side]
        own, other = balls[side], balls[side ^ 1]
        level = depth[side] + 1
        nxt, cands = [], 0
        for cur in fronts[side]:
            row = ci[rp[cur]:rp[cur + 1]].tolist()
            stats[4] += len(row)
            for nb in row:
                if nb in own:
                    continue
                own[nb] = (cur, level)
                stats[2 + side] += 1
                if nb in other:
                    cands += 1
                    if meet is None or other[nb][1] < meet[0]:
                        meet = (other[nb][1], nb)
                else:
                    nxt.append(nb)
        fronts[side] = nxt
        depth[side] = level
        stats[side] += 1
        stats[6] = cands
    m = meet[1]
    stats[5] = m
    path = [m]
    while path[-1] != src:
        path.append(balls[0][path[-1]][0])
    path.reverse()
    while path[-1] != dst:
        path.append(balls[1][path[-1]][0])
    return path, stats


def shortest_path(n, rows, cols, src, dst, max_hops=-1, undirected=False, prepared=None):
    tables = prepared if prepared is not None else prepare(n, rows, cols, undirected)
    return search(tables, src, dst, max_hops)


def type_order(edges, types, graph_types=None):
    """the types a pattern scans, in order: the named ones that exist, or every type in the graph's order (graph_types: the
    graph's types in creation order, when edges were deleted since and first appearance no longer tells)"""
    have = list(dict.fromkeys(ty for _, ty, _, _ in edges)) if graph_types is None else list(graph_types)
    return [t for t in types if t in have] if types else have


def reference_path(edges, src, dst, types, directed=True, min_hops=1, max_hops=None, graph_types=None):
    if src is None or dst is None:
        return None
    if min_hops == 0 and src == dst:
        return [src], []
    order = type_order(edges, types, graph_types)
    scan = [(i, ty, s, d) for i, ty, s, d in edges if ty in order]
    n = max([-1] + [max(s, d) for _, _, s, d in scan]) + 1
    if src >= n or dst >= n:   # (an id no edge names — past the capacity, say — has no neighbour)
        return None
    tables = prepare(n, [s for _, _, s, _ in scan], [d for _, _, _, d in scan], not directed)
    path, _ = search(tables, src, dst, -1 if max_hops is None else max_hops)
    if path is None or len(path) - 1 < min_hops:
        return None
    ids = []
    for u, v in zip(path, path[1:]):
        for a, b in ((u, v), (v, u)):
            hit = [i for t in order for i in sorted(i for i, ty, s, d in scan if ty == t and (s, d) == (a, b))]
            if hit:
                ids.append(hit[0])
                break
    return path, ids
