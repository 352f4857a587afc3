"""GPU: algo.MSF, algo.SPpaths and the pruning table of algo.SPpaths' enumeration through the host layer, whose weight matrix the
device builds (fgpu_pair_weights over the tensors' own layers): a generated multigraph with two types, parallel edges, unlisted
ids and pending deletions / additions against the plain-Python expectations the host tests use — the pair rule restated, then
the Kruskal / Dijkstra / enumeration checkers — kept relationship ids included.  The attribute lists arrive unsorted and with a
repeated id, and after every call Graph.pair_stats() shows that the device built the matrix."""
import math
import os
import sys

import numpy as np
import pytest

from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_weights_check as pw  # noqa: E402
import sppaths_enum_check as enum  # noqa: E402
from msf_check import bits_of, msf  # noqa: E402
from sssp_check import sssp  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
N = 300
DIRECTION = {"outgoing": pw.OUT, "incoming": pw.IN, "both": pw.OUT | pw.IN}
REVERSE = {"outgoing": pw.IN, "incoming": pw.OUT, "both": pw.OUT | pw.IN}


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(hctx):
    """(graph, effective edges (type, src, dst, id), label membership, scores for algo.MSF, weights for the paths, costs)"""
    rng = np.random.default_rng(29)
    g = host.Graph(hctx, N)
    lab = {name: g.add_label(name) for name in ("P", "Q")}
    typ = {name: g.add_type(name) for name in ("A", "B")}
    has = {name: rng.random(N) < p for name, p in (("P", 0.5), ("Q", 0.3))}
    for name, m in has.items():
        for v in np.flatnonzero(m):
            g.label_node(int(v), lab[name])
    edges = []

    def add(eid):
        t = ("A", "B")[int(rng.integers(0, 2))]
        a, b = (int(x) for x in rng.integers(0, N, 2))
        if eid % 4 == 0 and edges:                              # a parallel edge, either direction, either type
            _, a, b, _ = edges[int(rng.integers(0, len(edges)))]
            if eid % 8 == 0:
                a, b = b, a
        edges.append((t, a, b, eid))
        g.create_edge(typ[t], a, b, eid)

    for eid in range(700):
        add(eid)
    g.commit()
    doomed = [edges[i] for i in rng.choice(len(edges), 120, replace=False)]   # pending deletions ...
    for t, a, b, eid in doomed:
        g.delete_edge(typ[t], a, b, eid)
    gone = {e[3] for e in doomed}
    edges[:] = [e for e in edges if e[3] not in gone]
    for eid in range(700, 850):                                               # ... and pending additions
        add(eid)
    ids = [e[3] for e in edges]
    scores = {i: [0.0, -0.0, 1.0, 2.5, -4.0, 7, 7.0, 1e300][int(rng.integers(0, 8))] for i in ids if i % 3}
    weights = {i: [0.0, -0.0, 0.5, 1.0, 2.5, 7.0, math.inf, math.nan][int(rng.integers(0, 8))] for i in ids if i % 3 != 1}
    costs = {i: float(rng.integers(1, 5)) for i in ids if i % 5}
    return g, edges, has, scores, weights, costs


def shuffled(attr, seed):
    """the attribute as pairs in a shuffled order, every seventh id once more in front with another value: the last one stands"""
    rng = np.random.default_rng(seed)
    pairs = [(k, v) for k, v in attr.items()]
    rng.shuffle(pairs)
    return [(k, 99.0) for k, _ in pairs[::7]] + pairs


def expected_trees(n, edges, selected, types, maximize, weights):
    """the pair rule in plain Python, then the checker.  edges: (type, src, dst, id) effective relationships"""
    best = {}
    for t, a, b, eid in edges:
        if (types and t not in types) or a == b or not (selected[a] and selected[b]):
            continue
        if weights is None:
            s = 1.0
        elif eid not in weights:
            s = math.inf
        else:
            s = -float(weights[eid]) if maximize else float(weights[eid])
        key = (min(a, b), max(a, b))
        if key not in best or s < best[key][0] or (s == best[key][0] and eid < best[key][1]):
            best[key] = (s, eid)
    lo = np.array([k[0] for k in best], dtype=np.int64)
    hi = np.array([k[1] for k in best], dtype=np.int64)
    b = bits_of(np.array([best[k][0] for k in best], dtype=np.float64))
    fr, fc, _, comp = msf(n, np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([b, b]), selected)
    trees = {}
    for v in np.flatnonzero(selected):
        trees.setdefault(int(comp[v]), ([], []))[0].append(int(v))
    for a, c in zip(fr.tolist(), fc.tolist()):
        trees[int(comp[a])][1].append(best[(a, c)][1])
    return [trees[k] for k in sorted(trees)], 2 * len(best)


def test_algo_msf(world):
    g, edges, has, scores, _, _ = world
    runs = 0
    for labels in [(), ("P",), ("P", "Q")]:
        selected = np.ones(N, dtype=bool)
        if labels:
            selected = np.zeros(N, dtype=bool)
            for name in labels:
                selected |= has[name]
        for types in [(), ("A",), ("B",)]:
            for maximize in (False, True):
                for w in (scores, None):
                    if w is None and maximize:
                        continue
                    want, n_pairs = expected_trees(N, edges, selected, types, maximize, w)
                    got = g.algo_msf(list(labels), list(types), maximize, None if w is None else shuffled(w, runs))
                    assert [(a.tolist(), b.tolist()) for a, b in got] == [(a, b) for a, b in want]
                    st = g.pair_stats()
                    rels = [e for e in edges if not types or e[0] in types]
                    flags = pw.OUT | pw.IN | (pw.NEGATE if maximize else 0)
                    assert st == pw.pair_weights(N, rels, w, flags, selected, math.inf)[4]
                    assert st[2] > 0 and st[3] == n_pairs
                    runs += 1
    assert runs == 27


def pair_matrix(edges, types, flags, weights):
    rels = [e for e in edges if not types or e[0] in types]
    return pw.pair_weights(N, rels, weights, flags | pw.DROP_NONFINITE | pw.REFUSE_NEGATIVE, None, 1.0)


@pytest.mark.parametrize("direction", ["outgoing", "incoming", "both"])
def test_algo_sp_paths(world, direction):
    g, edges, _, _, weights, costs = world
    for types, w in (((), weights), (("A",), weights), (("B", "A", "B"), None)):
        rows, cols, bits, kept, stats = pair_matrix(edges, types, DIRECTION[direction], w)
        kept_of = {(int(r), int(c)): int(k) for r, c, k in zip(rows, cols, kept)}
        for s in (0, 17, 101):
            dist, parent, _ = sssp(N, rows, cols, bits, s)
            for t in range(1, N, 7):
                got = g.algo_sp_paths(s, t, list(types), direction, None if w is None else shuffled(w, t), shuffled(costs, s))
                assert g.pair_stats() == stats and stats[2] > 0 and stats[3] == len(rows)
                if t == s or not np.isfinite(dist[t]):
                    assert got is None
                    continue
                nodes, rels, weight, cost = got
                chain = [t]
                while chain[-1] != s:
                    chain.append(int(parent[chain[-1]]))
                chain.reverse()
                assert list(nodes) == chain and np.float64(weight).view(U64) == dist[t].view(U64)
                assert list(rels) == [kept_of[(a, b)] for a, b in zip(chain, chain[1:])]
                assert cost == sum(costs.get(e, 0.0) for e in rels)


@pytest.mark.parametrize("direction", ["outgoing", "incoming", "both"])
def test_algo_sp_paths_rows(world, direction):
    g, edges, _, _, weights, costs = world
    listed = [(i, t, s, d) for t, s, d, i in edges]
    finite = {k: v for k, v in weights.items() if math.isfinite(v)}   # (the walk adds the weights up: keep the sums finite)
    calls = 0
    for types, path_count, max_len in (((), 2, 3), (("A",), 0, 4), (("B",), 5, 3)):
        stats = pair_matrix(edges, types, REVERSE[direction], finite)[4]
        for s, t in ((0, 17), (5, 200), (101, 33), (250, 9)):
            want = enum.paths(listed, ["A", "B"], N, s, t, types, direction, max_len, None, path_count, finite, costs, prune=True)
            got = g.algo_sp_paths_rows(s, t, list(types), direction, max_len, None, path_count, shuffled(finite, s), shuffled(costs, t))
            assert [(r[1].tolist(), r[0].tolist(), r[2], r[3]) for r in got] == [(e, nd, w, c) for e, nd, w, c in want]
            assert g.pair_stats() == stats and stats[2] > 0
            calls += 1
    assert calls == 12


def test_the_negative_weight_message_names_the_relationship(world):
    g, edges, _, _, weights, _ = world
    ids = sorted(e[3] for e in edges if e[1] != e[2])
    bad = dict(weights)
    bad[ids[40]] = -2.0
    bad[ids[5]] = -0.25
    for call in (lambda: g.algo_sp_paths(0, 17, weights=shuffled(bad, 1)),
                 lambda: g.algo_sp_paths(0, 17, direction="both", weights=bad)):
        with pytest.raises(host.HostError) as e:
            call()
        assert f"algo.SPpaths: relationship {ids[5]} has a negative weight" in str(e.value)
    assert g.pair_stats() == [0] * 8
    loop = [e for e in edges if e[1] == e[2]]                     # a self-loop's negative weight is not refused
    if loop:
        ok = dict(weights)
        ok[loop[0][3]] = -1.0
        g.algo_sp_paths(0, 17, weights=ok)
    g.algo_msf((), (), True, bad)                                 # algo.MSF refuses nothing
    assert g.pair_stats()[2] > 0
