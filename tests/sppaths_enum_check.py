"""Checker for fgpu_sssp_hops and for the enumeration shapes of algo.SPpaths / algo.SSpaths (no GPU, no engine import): the rules
of include/fgpu.h and the reference's enumerate_paths / record_found_path / final sort (algo_procedures.rs:2350-2597, cited as
:line below) restated in plain Python.

hop_table(n, rows, cols, bits, src, max_hops) -> (table float64[max_hops + 1, n], stats)
    D_0[src] = +0.0, +inf elsewhere; D_h[v] = min(D_{h-1}[v], min over entries (u, v), u != v, of D_{h-1}[u] + W(u, v) where that
    sum is finite), every round from D_{h-1} alone (numpy, bit-exact: one IEEE addition per entry and a minimum).  bits: binary64
    patterns per entry, None = every weight 1.0; -0.0 is 0.0; a NaN or a negative weight raises ValueError.  stats = [rounds whose
    frontier was not empty, frontier entries taken, entries read, first h with D_h == D_{h-1} or max_hops + 1], the frontier of
    round 1 being {src} and of round h + 1 the vertices round h lowered.  (rows, cols) pairs must be distinct.

successors(edges, order, node, direction) -> [(edge id, edge src, edge dst, far end), ...]
    node_successors (:2098-2109) over get_node_relationships_by_type (graph.rs:1797-1835), the adjacency order asp_check.py
    states: per type of `order` the outgoing half by (dst, id), then the incoming half by (src, id) without the self-loops the
    outgoing half gave.  edges: [(id, type, src, dst), ...].

type_order(edges_types, types) -> the tensors a relTypes list selects: [] = every type in creation order, else the known names in
    the order listed — a name listed twice is there twice (filter_map, graph.rs:1803-1810), and so are its successors.

paths(edges, all_types, n, source, target, types, direction, max_len, max_cost, path_count, weights, costs, prune, max_examined,
      stats) -> [(edge ids, nodes, weight, cost), ...]
    run_path_algo's enumeration branch (:2573-2596); target None = algo.SSpaths.  max_len None = no maxLen.  weights / costs:
    None = no weightProp / costProp, else {edge id: number} (missing: 1.0 / 0.0).  prune: the walk skips the successors the
    hop-bounded table from the target rules out (the host layer's rule, host.hpp); the rows must not depend on it.  stats: a
    dict that receives examined / pruned_hops / pruned_weight / table_rows.  The unpruned walk seeds its bound with +inf: the
    rows do not depend on the seed as long as it is at least the weight of a cheapest qualifying path."""
import bisect
import math

import numpy as np

U64 = np.uint64
NEG0 = 0x8000000000000000
HOPS_MAX = 32
TABLE_BYTES_MAX = 1 << 30


def _weights(bits, m):
    if bits is None:
        return np.ones(m, dtype=np.float64)
    b = np.asarray(bits, dtype=U64).copy()
    b[b == U64(NEG0)] = U64(0)
    w = b.view(np.float64)
    if np.isnan(w).any() or (b >> U64(63)).any():
        raise ValueError("a weight is NaN or negative")
    return w


def hop_table(n, rows, cols, bits, src, max_hops):
    rows, cols = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
    w = _weights(bits, len(rows))
    deg = np.bincount(rows, minlength=n) if n else np.zeros(0, dtype=np.int64)
    off = rows != cols
    r, c, w = rows[off], cols[off], w[off]
    table = np.full((max_hops + 1, n), np.inf, dtype=np.float64)
    table[0, src] = 0.0
    frontier = np.array([src], dtype=np.int64)
    rounds = popped = read = 0
    fixed = max_hops + 1
    for h in range(1, max_hops + 1):
        prev = table[h - 1]
        cur = prev.copy()
        if len(frontier):
            rounds += 1
            popped += len(frontier)
            read += int(deg[frontier].sum())
        with np.errstate(over="ignore"):
            cand = prev[r] + w
        ok = np.isfinite(cand)
        np.minimum.at(cur, c[ok], cand[ok])
        table[h] = cur
        frontier = np.nonzero(cur.view(U64) != prev.view(U64))[0]
        if not len(frontier) and fixed > max_hops:
            fixed = h
    return table, [rounds, popped, read, fixed]


def _relax_once(prev, rows, cols, bits):
    """one round of the recurrence from an arbitrary row"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    w = _weights(bits, len(rows))
    cur = prev.copy()
    with np.errstate(over="ignore"):
        cand = prev[rows] + w
    ok = np.isfinite(cand) & (rows != cols)
    np.minimum.at(cur, cols[ok], cand[ok])
    return cur


def index_edges(edges):
    """edges by (type, src) and by (type, dst): successors' `edges` argument for many calls on one graph"""
    by_src, by_dst = {}, {}
    for i, ty, s, d in edges:
        by_src.setdefault((ty, s), []).append((d, i, s))
        by_dst.setdefault((ty, d), []).append((s, i, d))
    for lst in list(by_src.values()) + list(by_dst.values()):
        lst.sort()
    return by_src, by_dst


def successors(edges, order, node, direction):
    by_src, by_dst = edges if isinstance(edges, tuple) else index_edges(edges)
    out, inc = direction in ("outgoing", "both"), direction in ("incoming", "both")
    seq = []
    for t in order:
        if out:
            seq += [(i, s, d, d) for d, i, s in by_src.get((t, node), ())]
        if inc:
            seq += [(i, s, d, s) for s, i, d in by_dst.get((t, node), ()) if not (out and s == node)]
    return seq


def type_order(all_types, types):
    return list(all_types) if not types else [t for t in types if t in all_types]


def _attr(d, i, default):
    return default if d is None else float(d.get(i, default))


def reverse_pair_weights(edges, order, direction, weights):
    """the smallest weight per ordered pair (from, to) in the REVERSE traversal direction, self-loops and non-finite weights
    left out; a negative weight among the selected relationships raises ValueError (host.hpp)"""
    best = {}
    sel = set(order)
    for i, ty, s, d in edges:
        if ty not in sel or s == d:
            continue
        w = _attr(weights, i, 1.0)
        if not math.isfinite(w):
            continue
        if w < 0.0:
            raise ValueError(f"relationship {i} has a negative weight")
        if w == 0.0:
            w = 0.0                      # (-0.0)
        pairs = []
        if direction != "outgoing":      # reversed: Incoming walks dst -> src, so its reverse is src -> dst
            pairs.append((s, d))
        if direction != "incoming":
            pairs.append((d, s))
        for p in pairs:
            if p not in best or w < best[p]:
                best[p] = w
    return best


def _record(results, found, path_count, bound):
    """record_found_path (:2350-2403); found = (key, edges, nodes), key = (weight, cost, hops); returns the new bound"""
    key = found[0]
    if path_count == 1:
        if not results or key < results[0][0]:
            results[:] = [found]
            return key[0]
        return bound
    if path_count == 0:
        if not results:
            results.append(found)
            return key[0]
        best = results[0][0][0]
        if key[0] > best:
            return bound
        if key[0] < best:
            results[:] = [found]
            return key[0]
        results.append(found)
        return bound
    k = path_count
    if len(results) == k:
        if not key < results[k - 1][0]:
            return bound
        results.pop()
    pos = bisect.bisect_left([r[0] for r in results], key)   # partition_point(kept < found): in front of its equals
    results.insert(pos, found)
    if len(results) == k:
        return results[k - 1][0][0]
    return bound


def paths(edges, all_types, n, source, target, types=(), direction="outgoing", max_len=None, max_cost=None, path_count=1,
          weights=None, costs=None, prune=False, max_examined=0, stats=None, deleted=()):
    if path_count < 0:
        raise ValueError("pathCount must be a non-negative integer")   # :1940
    st = {"examined": 0, "pruned_hops": 0, "pruned_weight": 0, "table_rows": -1}
    if stats is not None:
        stats.clear()
        stats.update(st)
        st = stats
    order = type_order(all_types, list(types))
    rev = reverse_pair_weights(edges, order, direction, weights)   # (raises on a negative weight, pruning or not)
    ML = 0xFFFFFFFF if max_len is None else max_len
    bound = math.inf
    slack = 0.0
    exact = False
    if source >= n or (target is not None and target >= n) or source in deleted or target in deleted:
        return []                            # (a deleted node has no relationship: only the early answer is modelled)
    if source == target:
        return []                            # bfs_find_bound never "finds" the source it starts from: None (:2278-2279)
    pruning = target is not None and prune
    if pruning:
        keys = sorted(rev)
        rr, cc = [k[0] for k in keys], [k[1] for k in keys]
        bits = None if weights is None else np.array([rev[k] for k in keys], dtype=np.float64).view(U64)
        if ML <= HOPS_MAX and (ML + 1) * n * 8 <= TABLE_BYTES_MAX:
            table, _ = hop_table(n, rr, cc, bits, target, ML)
            st["table_rows"] = ML + 1
            row_of = lambda left: table[left]
        else:
            full = np.full(n, np.inf)    # fgpu_sssp's dist: the fixed point of the same recurrence, at most n - 1 rounds away
            full[target] = 0.0
            for _ in range(n):
                nxt = _relax_once(full, rr, cc, bits)
                if np.array_equal(nxt.view(U64), full.view(U64)):
                    break
                full = nxt
            st["table_rows"] = 0
            row_of = lambda left: full
        m = min(ML, max(n - 1, 0)) + 1
        slack = 8.0 * m * 2.0 ** -53
        reach = row_of(ML)[source]
        if math.isinf(reach):
            return []
        # the fallback's one row knows no hop budget: it may prune, but it is a qualifying path's weight (a seed, and the
        # answer to "is there a route within maxLen") only when no simple path is longer than maxLen anyway
        exact = st["table_rows"] > 0 or ML >= n - 1
        if exact and path_count in (0, 1) and max_cost is None:
            bound = reach * (1.0 + slack)
    results = []
    index = index_edges(edges)
    if target is not None and not (pruning and exact):   # bfs_find_bound's None (:2267-2320): no route within maxLen, no walk
        seen, frontier, found = {source}, [source], False
        for _ in range(min(ML, n)):
            nxt = []
            for u in frontier:
                for _, _, _, far in successors(index, order, u, direction):
                    if far not in seen:
                        seen.add(far)
                        nxt.append(far)
            found = found or target in nxt
            frontier = nxt
            if found or not frontier:
                break
        if not found:
            return []
    nodes, live, on_path = [source], [], {source}   # live: (edge id, prefix weight, prefix cost)
    levels = [successors(index, order, source, direction) if ML > 0 else None]
    while True:
        depth = len(live)
        lv = levels[depth]
        if lv:
            eid, _, _, nxt = lv.pop()
            st["examined"] += 1
            if max_examined and st["examined"] > max_examined:
                raise RuntimeError("the enumeration spent its budget of examined successors")
            if nxt in on_path:
                continue
            w0, c0 = (live[-1][1], live[-1][2]) if live else (0.0, 0.0)
            nw = w0 + _attr(weights, eid, 1.0)
            nc = c0 + _attr(costs, eid, 0.0)
            if not math.isfinite(nw) or nw > bound:
                continue
            if not math.isfinite(nc) or (max_cost is not None and nc > max_cost):
                continue
            if pruning:
                L = row_of(ML - (depth + 1))[nxt]
                if math.isinf(L):
                    st["pruned_hops"] += 1
                    continue
                if (nw + L) * (1.0 - slack) > bound:
                    st["pruned_weight"] += 1
                    continue
            live.append((eid, nw, nc))
            nodes.append(nxt)
            on_path.add(nxt)
            at_target = target is None or nxt == target
            if at_target:
                bound = _record(results, ((nw, nc, len(live)), [e[0] for e in live], list(nodes)), path_count, bound)
            expand = not (at_target and target is not None) and len(live) < ML
            levels.append(successors(index, order, nxt, direction) if expand else None)
        else:
            if depth == 0:
                break
            levels.pop()
            live.pop()
            on_path.discard(nodes.pop())
    results.sort(key=lambda r: r[0])   # (stable: cmp_found_path, :2037-2045)
    return [(e, nd, key[0], key[1]) for key, e, nd in results]


# ---- the seeded cases of the tests (CPU: pruned against unpruned; GPU: the host layer against this checker) ------------------
DIRECTIONS = ("outgoing", "incoming", "both")
REL_TYPES = ((), ("R",), ("R", "S"), ("nope",), ("S", "S"))   # empty / one / both / an unknown name / one name listed twice
MAX_LENS = (0, 1, 3, 6, None)
MAX_COSTS = (None, 4, 1000)                                   # none / tight (costs are 1 .. 4 per relationship) / loose
PATH_COUNTS = (0, 1, 2, 5)
SEEDS = tuple(range(12))
CALLS_PER_SEED = 45


def seeded_graph(seed):
    """8 .. 40 nodes of which the last is deleted (it never had a relationship), two relationship types, multi-edges and
    self-loops; even seeds weigh 0.1 / 0.2 / 0.3 / 0.5 / 0.7 / 0.0, odd seeds small integers, a fifth of the relationships is
    not listed (1.0), every sixth seed has no weightProp; integer costs 1 .. 4.  Sparse on purpose: m = 2.2 n keeps the
    unbounded, unpruned walks of seeded_calls within a few thousand steps (7 230 at most).
    Returns (n, edges [(id, type, src, dst)], weights | None, costs)."""
    import random

    from asp_check import random_multigraph
    rng = random.Random(0x5EED0 + seed)
    n = rng.randrange(8, 41)
    edges = random_multigraph(rng, n - 1, int(2.2 * n), ["R", "S"])
    pool = (0.1, 0.2, 0.3, 0.5, 0.7, 0.0) if seed % 2 == 0 else (0.0, 1.0, 2.0, 3.0, 4.0)
    weights = None if seed % 6 == 5 else {i: rng.choice(pool) for i, _, _, _ in edges if rng.random() < 0.8}
    costs = {i: float(rng.randrange(1, 5)) for i, _, _, _ in edges}
    return n, edges, weights, costs


def seeded_calls(seed):
    """CALLS_PER_SEED calls on seeded_graph(seed): (source, target, kwargs) with kwargs for paths() — every value of every
    swept axis occurs (test_sppaths_enum_cpu.py checks that)"""
    import random
    rng = random.Random(0xCA115 + seed)
    n, edges, _, _ = seeded_graph(seed)
    ends = sorted({s for _, _, s, _ in edges} | {d for _, _, _, d in edges})
    near = {}
    for _, _, s, d in edges:
        near.setdefault(s, set()).add(d)
        near.setdefault(d, set()).add(s)
    calls = []
    for i in range(CALLS_PER_SEED):
        source = rng.choice(ends)
        u = rng.random()
        if u < 0.05:
            target = source
        elif u < 0.08:
            target = n - 1                                   # the deleted node
        elif u < 0.7:                                        # one or two relationships away, in either direction
            target = rng.choice(sorted(near[source]))
            if rng.random() < 0.5:
                target = rng.choice(sorted(near[target]))
        else:
            target = rng.choice(ends)
        j = i + seed
        calls.append((source, target, {"types": REL_TYPES[j % 5], "direction": DIRECTIONS[(j // 5) % 3], "max_len": MAX_LENS[(j // 2) % 5],
                                       "max_cost": MAX_COSTS[(j // 7) % 3], "path_count": PATH_COUNTS[(j // 3) % 4]}))
    return calls


def is_fast_shape(source, target, kw):
    return kw["path_count"] == 1 and kw["max_len"] is None and kw["max_cost"] is None and source != target


def detour_graph(k=35):
    """the chain 0 -> 1 -> ... -> k at 1.0 each plus the arc 0 -> k at 100.0: the cheapest route needs k arcs, so under a
    maxLen below k the hop-limited optimum (100.0) is heavier than the unbounded one (k).  Returns (n, edges, weights)."""
    edges = [(i, "R", i, i + 1) for i in range(k)] + [(k, "R", 0, k)]
    weights = {i: 1.0 for i in range(k)}
    weights[k] = 100.0
    return k + 1, edges, weights
