"""CPU side of the max-flow tests.  certify() proves that a returned flow is a MAXIMUM flow without a second solver having to
agree on the assignment (which is not unique): it checks the rules include/fgpu.h writes down for fgpu_maxflow — every entry an
arc of C with 0 < f <= cap, at most one direction per arc pair, conservation, the value at src and sink — and then that a BFS
from src over the residual graph of that flow does not reach sink.  By max-flow / min-cut that is complete.  dinic() is a plain
Dinic that returns the value only.  tests/test_maxflow_cpu.py holds both against hand cases and broken flows."""
from collections import deque

import numpy as np


def live_arcs(rows, cols, caps):
    """{(u, v): capacity} of the arcs that count: off the diagonal, capacity > 0 (-0.0 and negatives are ignored)"""
    arcs = {}
    for u, v, c in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(caps, dtype=np.float64).tolist()):
        if u != v and c > 0.0:
            assert (u, v) not in arcs, "the test matrices hold one entry per position"
            arcs[(int(u), int(v))] = c
    return arcs


def certify(n, rows, cols, caps, src, sink, value, frows, fcols, fvals, exact=True, tol=0.0):
    """Raises AssertionError unless (frows, fcols, fvals) is a maximum src -> sink flow of `value` in the network C.  exact=True:
    every comparison is equality (integer or dyadic capacities).  exact=False: conservation and the value hold to `tol`, and an
    arc counts as residual when more than `tol` of it is left."""
    if exact:
        tol = 0.0
    arcs = live_arcs(rows, cols, caps)
    frows = np.asarray(frows).astype(np.int64).tolist()
    fcols = np.asarray(fcols).astype(np.int64).tolist()
    fvals = np.asarray(fvals, dtype=np.float64).tolist()
    assert len(frows) == len(fcols) == len(fvals)
    assert sorted(zip(frows, fcols)) == list(zip(frows, fcols)), "flow entries are not sorted by (row, col)"
    flow = {}
    net = np.zeros(n, dtype=np.float64)   # outflow - inflow; exact for the capacities the exact tests use
    for u, v, f in zip(frows, fcols, fvals):
        assert (u, v) in arcs, f"flow on ({u}, {v}), which is not a live arc of C"
        assert (u, v) not in flow, f"({u}, {v}) returned twice"
        assert 0.0 < f <= arcs[(u, v)], f"flow {f} on ({u}, {v}) with capacity {arcs[(u, v)]}"
        assert (v, u) not in flow, f"both ({u}, {v}) and ({v}, {u}) carry flow"
        flow[(u, v)] = f
        net[u] += f
        net[v] -= f
    inner = np.ones(n, dtype=bool)
    inner[[src, sink]] = False
    worst = float(np.abs(net[inner]).max()) if inner.any() else 0.0
    assert worst <= tol, f"conservation broken by {worst}: this is a preflow, not a flow"
    assert abs(net[src] - value) <= tol, f"net outflow of src {net[src]} != value {value}"
    assert abs(-net[sink] - value) <= tol, f"net inflow of sink {-net[sink]} != value {value}"
    # residual graph: u -> v when cap - f > tol, v -> u when f > tol
    adj = [[] for _ in range(n)]
    for (u, v), c in arcs.items():
        f = flow.get((u, v), 0.0)
        if c - f > tol:
            adj[u].append(v)
        if f > tol:
            adj[v].append(u)
    seen = np.zeros(n, dtype=bool)
    seen[src] = True
    q = deque([src])
    while q:
        u = q.popleft()
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                q.append(v)
    assert not seen[sink], "an augmenting path is left: the flow is not maximal"
    return net


def dinic(n, rows, cols, caps, src, sink):
    """the value of a maximum src -> sink flow (Dinic, iterative); capacities as certify() reads them"""
    arcs = live_arcs(rows, cols, caps)
    head, nxt, to, res = [-1] * n, [], [], []
    for (u, v), c in arcs.items():
        for a, b, x in ((u, v, c), (v, u, 0.0)):
            to.append(b)
            res.append(x)
            nxt.append(head[a])
            head[a] = len(to) - 1
    total = 0.0
    while True:
        level = [-1] * n
        level[src] = 0
        q = deque([src])
        while q:
            u = q.popleft()
            e = head[u]
            while e != -1:
                if res[e] > 0.0 and level[to[e]] < 0:
                    level[to[e]] = level[u] + 1
                    q.append(to[e])
                e = nxt[e]
        if level[sink] < 0:
            return total
        it = list(head)
        while True:   # one augmenting path of the level graph per turn
            path, u = [], src
            while u != sink:
                e = it[u]
                while e != -1 and not (res[e] > 0.0 and level[to[e]] == level[u] + 1):
                    e = nxt[e]
                it[u] = e
                if e == -1:
                    if not path:
                        break
                    level[u] = -1   # dead end: retreat
                    u = to[path.pop() ^ 1]
                    continue
                path.append(e)
                u = to[e]
            if u != sink:
                break
            d = min(res[e] for e in path)
            for e in path:
                res[e] -= d
                res[e ^ 1] += d
            total += d
