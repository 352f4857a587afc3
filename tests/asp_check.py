"""Checker for fgpu_shortest_dag and Graph.all_shortest_paths (no GPU, no engine import): the rules of include/fgpu.h and the
reference's AllShortestPathsOp restated in plain Python.

shortest_dag(n, rows, cols, src, dst, max_hops, prepared=None) -> (L, [(from, to, depth), ...])
    One-sided, on the pattern: d(src, .) by a BFS over the entries, d(., dst) by a BFS over the reversed entries, then
      src != dst   L = d(src, dst)
      src == dst   L = 1 + the least d(src, u) over the entries u -> src (u = src at 0 for a self-loop)
    and the pairs (u, v) with an entry u -> v and d(src, u) + 1 + d(v, dst) == L, sorted, depth = d(src, u).  L = -1 and no
    pair when there is no path or L > max_hops (max_hops < 0: unbounded; 0: never a path).

reference_paths(nodes, edges, src, dst, types, bidirectional, reversed, max_hops) -> [[edge id, ...], ...]
    The operator's queue BFS and LIFO DFS (runtime/ops/all_shortest_paths.rs, cited as :line below) over an edge list.
    nodes: the node count; edges: [(id, type, src, dst), ...]; types: the pattern's type names in order ([] = every type, in
    the order the types first appear in `edges`: the order their matrices were created in); max_hops None = unbounded.
    Returns the paths as lists of relationship ids, in the order the operator emits them and in its per-path edge order.
    min_hops is always 1 (the parser refuses anything else: cypher.rs:1324-1331); attribute filters are not modelled.

path_count(L, pairs, src, dst, mult=None) -> the number of src -> dst walks through the DAG, by dynamic programming over the
    depths; mult[(u, v)] (default 1) = the relationships that stand behind the pattern pair."""
from collections import deque

import numpy as np


def prepare(n, rows, cols):
    """the pattern as two CSRs (entries and reversed entries), duplicates dropped: shortest_dag's `prepared` argument, for
    several calls on one graph"""
    rows, cols = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
    both = []
    for a, b in ((rows, cols), (cols, rows)):
        key = np.unique(a * n + b)
        r, c = key // n, key % n
        rp = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
        both.append((rp, c, r))
    return both


def _bfs(n, rp, ci, start):
    dist = np.full(n, -1, dtype=np.int64)
    dist[start] = 0
    frontier = np.array([start], dtype=np.int64)
    d = 0
    while len(frontier):
        d += 1
        b, e = rp[frontier], rp[frontier + 1]
        ln = e - b
        pos = np.repeat(b - np.concatenate(([0], np.cumsum(ln)[:-1])), ln) + np.arange(int(ln.sum()))
        nxt = np.unique(ci[pos])
        frontier = nxt[dist[nxt] < 0]
        dist[frontier] = d
    return dist


def shortest_dag(n, rows, cols, src, dst, max_hops=-1, prepared=None):
    (rp, ci, ri), (rpt, cit, _) = prepared if prepared is not None else prepare(n, rows, cols)
    df = _bfs(n, rp, ci, src)
    db = _bfs(n, rpt, cit, dst)
    if src != dst:
        L = int(df[dst])
    else:
        closers = df[cit[rpt[src]:rpt[src + 1]]]
        closers = closers[closers >= 0]
        L = 1 + int(closers.min()) if len(closers) else -1
    if L < 1 or (max_hops >= 0 and L > max_hops):
        return -1, []
    keep = (df[ri] >= 0) & (db[ci] >= 0) & (df[ri] + 1 + db[ci] == L)
    return L, list(zip(ri[keep].tolist(), ci[keep].tolist(), df[ri[keep]].tolist()))


def node_relationships(edges, order, node, bidirectional):
    """get_node_relationships_by_type (graph.rs:1797-1835): per type in order, the outgoing half by (dst, id), then — for
    EdgeDirection::Both — the incoming half by (src, id) without the self-loops the outgoing half already gave"""
    seq = []
    for t in order:
        seq += sorted(((d, i, s) for i, ty, s, d in edges if ty == t and s == node), key=lambda e: (e[0], e[1]))
        if bidirectional:
            seq += [(d, i, s) for s, i, d in sorted((s, i, d) for i, ty, s, d in edges if ty == t and d == node and s != node)]
    return [(s, d, i) for d, i, s in seq]   # (edge src, edge dst, edge id)


def reference_paths(nodes, edges, src, dst, types, bidirectional, reversed, max_hops=None):
    order = []
    for t in (types if types else [ty for _, ty, _, _ in edges]):
        if t not in order and any(ty == t for _, ty, _, _ in edges):   # (unknown names are dropped: filter_map, graph.rs:1806-1809)
            order.append(t)
    max_hops = 0xFFFFFFFF if max_hops is None else max_hops   # :123
    pred, dist = {}, {src: 0}                                  # :130-131, :138
    queue = deque([src])                                       # :139
    is_cycle = src == dst                                      # :136
    shortest = None                                            # :141
    while queue:                                               # :143
        cur = queue.popleft()
        cd = dist[cur]
        if shortest is not None and cd >= shortest:            # :147-151
            continue
        if cd >= max_hops:                                     # :153-155
            continue
        for es, ed, eid in node_relationships(edges, order, cur, bidirectional):   # :163-164
            if es == cur:                                      # :166-184 (both arms take the edge from its source first)
                nxt = ed
            elif bidirectional and ed == cur:
                nxt = es
            else:
                continue
            nd = cd + 1                                        # :207
            if is_cycle and nxt == src:                        # :212-235 (min_hops is 1: next_dist < min_hops never holds)
                if shortest is None:
                    shortest = nd
                    pred.setdefault(nxt, []).append((cur, eid))
                elif nd == shortest:
                    pred.setdefault(nxt, []).append((cur, eid))
                continue
            if nxt in dist:                                    # :237-245
                if nd == dist[nxt]:
                    pred.setdefault(nxt, []).append((cur, eid))
            else:                                              # :246-260
                dist[nxt] = nd
                pred.setdefault(nxt, []).append((cur, eid))
                if nxt == dst:
                    shortest = nd
                if nd < max_hops:
                    queue.append(nxt)
    if dst not in pred:                                        # :265-267
        return []
    out = []
    stack = [(dst, [])]                                        # :275
    while stack:                                               # :278-299
        node, path = stack.pop()
        if node == src and path:
            p = list(path)
            if not is_cycle:
                p.reverse()                                    # :281-285
            if reversed:
                p.reverse()                                    # :286-288
            out.append(p)
            continue
        for prev, eid in pred.get(node, []):
            stack.append((prev, path + [eid]))
    return out


def pairs_of_paths(paths, edges, bidirectional, src, is_cycle, reversed):
    """the (from, to) pattern pairs the returned paths traverse, oriented along the walk from src; sorted, each once"""
    ends = {i: (s, d) for i, _, s, d in edges}
    got = set()
    for p in paths:
        walk = list(p)
        if reversed:
            walk.reverse()       # back to the operator's own order
        if is_cycle:
            walk.reverse()       # a cycle keeps the dst -> src predecessor chain: back to src -> dst
        at = src
        for eid in walk:
            s, d = ends[eid]
            if s == at:
                nxt = d
            else:
                assert bidirectional and d == at, (p, eid, at)
                nxt = s
            got.add((at, nxt))
            at = nxt
    return sorted(got)


def path_count(L, pairs, src, dst, mult=None):
    if L < 1:
        return 0
    ways = {(src, 0): 1}
    for depth in range(L):
        for u, v, d in pairs:
            if d == depth and (u, depth) in ways:
                ways[(v, depth + 1)] = ways.get((v, depth + 1), 0) + ways[(u, depth)] * (mult or {}).get((u, v), 1)
    return ways.get((dst, L), 0)


def random_multigraph(rng, n, m, types, loops=0.1, repeat=0.25):
    """m relationships [(id, type, src, dst)] over n nodes from a random.Random: self-loops with probability `loops`, and with
    probability `repeat` a relationship joins a pair an earlier one joins already (same direction or opposite, any type)"""
    edges = []
    for i in range(m):
        if edges and rng.random() < repeat:
            _, _, s, d = rng.choice(edges)
            if rng.random() < 0.3:
                s, d = d, s
        elif rng.random() < loops:
            s = d = rng.randrange(n)
        else:
            s, d = rng.randrange(n), rng.randrange(n)
        edges.append((i, rng.choice(types), s, d))
    return edges


def pattern(edges, types, bidirectional):
    """the pattern matrix the operator hands to the device — the union over `types` ([] = all) of the adjacency, plus its
    transpose when bidirectional — as sorted (rows, cols), and the relationships behind every pair"""
    mult = {}
    for _, ty, s, d in edges:
        if types and ty not in types:
            continue
        mult[(s, d)] = mult.get((s, d), 0) + 1
        if bidirectional and s != d:
            mult[(d, s)] = mult.get((d, s), 0) + 1
    keys = sorted(mult)
    return [k[0] for k in keys], [k[1] for k in keys], mult
