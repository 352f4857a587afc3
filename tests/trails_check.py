"""The rule fgpu_expand_trails implements (falkordb_amd/csrc/expand_trails.hip), in plain Python over oracle.model graphs: a
level-synchronous trail expansion whose emission order comes from sums and prefix sums alone, no stack and no sort.

    E(F) = the emitting children of frame F          S(F) = E(F) + sum of S(c) over F's child frames
    base(root) = 0, or 1 after a 0-hop row           child frames c_0 .. c_j of F in adjacency order:
                                                         base(c_i) = base(F) + E(F) + sum of S(c_i') over i' > i
    F's emitting children land at base(F) .., in adjacency order.

tests/test_expand_trails_cpu.py holds it against model.var_len_expand, the LIFO DFS of the reference."""
from oracle import model


def level_expand(g, start, types=(), dest=None, min_hops=1, max_hops=None, reversed=False, bidirectional=False, dst_labels=(),
                 emit_path=False):
    """What model.var_len_expand returns for the same arguments: [(from, to, path | None)]."""
    lids, label_missing = [], False
    for l in dst_labels:
        if l in g.label_ids:
            lids.append(g.label_ids[l])
        else:
            label_missing = True
    node_ok = lambda v: (dest is None or dest == v) and not label_missing and all(g.node_has_label_id(v, l) for l in lids)
    zero = 1 if (min_hops == 0 and node_ok(start)) else 0
    w_out, w_in = bidirectional or not reversed, bidirectional or reversed

    # ---- the levels: frames = (node, parent index in the level above, edge that led here); a frame's children and its
    # emissions are contiguous, in adjacency order
    levels = [{"frames": [(start, None, None)]}]
    d = 0
    while levels[d]["frames"] and (max_hops is None or d + 1 <= max_hops):
        lv = levels[d]
        hop = d + 1
        child_beg, emit_beg, children, emits = [0], [0], [], []
        for f, (node, _, _) in enumerate(lv["frames"]):
            used, x = set(), f
            for l in range(d, 0, -1):                 # the trail: walk the parent links
                _, parent, edge = levels[l]["frames"][x]
                used.add(edge)
                x = parent
            for (s_, d_, e) in model.node_relationships(g, node, list(types), w_out, w_in):
                if e in used:
                    continue
                nb = s_ if reversed or s_ != node else d_
                if hop >= min_hops and node_ok(nb):
                    emits.append((f, nb, e))
                if max_hops is None or hop < max_hops:
                    children.append((nb, f, e))
            child_beg.append(len(children))
            emit_beg.append(len(emits))
        lv.update(child_beg=child_beg, emit_beg=emit_beg, emits=emits)
        levels.append({"frames": children})
        d += 1
    levels = [lv for lv in levels if "emits" in lv]

    # ---- S bottom-up: one segmented sum per level, through the prefix sums P of the level below
    below = None
    for lv in reversed_list(levels):
        nf = len(lv["frames"])
        S = [lv["emit_beg"][f + 1] - lv["emit_beg"][f] for f in range(nf)]
        if below is not None:
            for f in range(nf):
                S[f] += below[lv["child_beg"][f + 1]] - below[lv["child_beg"][f]]
        P = [0]
        for s in S:
            P.append(P[-1] + s)
        lv["P"] = below = P
    total = zero + (levels[0]["P"][-1] if levels else 0)

    # ---- base top-down: one segmented exclusive SUFFIX sum per level — the later siblings' subtrees run first
    out = [None] * total
    if zero:
        out[0] = (start, start, [start] if emit_path else None)
    for d, lv in enumerate(levels):
        if d == 0:
            lv["base"] = [zero]
        else:
            up = levels[d - 1]
            lv["base"] = [up["base"][p] + (up["emit_beg"][p + 1] - up["emit_beg"][p]) + lv["P"][up["child_beg"][p + 1]] - lv["P"][c + 1]
                          for c, (_, p, _) in enumerate(lv["frames"])]
        for j, (f, nb, e) in enumerate(lv["emits"]):
            o = lv["base"][f] + (j - lv["emit_beg"][f])
            path = None
            if emit_path:
                path, x = [nb, e], f
                for l in range(d, 0, -1):
                    node, parent, edge = levels[l]["frames"][x]
                    path += [node, edge]
                    x = parent
                path.append(start)
                if not reversed:
                    path.reverse()
            assert out[o] is None
            out[o] = (nb, start, path) if reversed else (start, nb, path)
    assert all(r is not None for r in out)
    return out


def reversed_list(xs):          # (the keyword argument `reversed` of level_expand shadows the builtin there)
    return xs[::-1]


def random_multigraph(rng, n=9, n_edges=16, acyclic=False):
    """A model.Graph with two types, two multi-edge pairs and (unless acyclic) self-loops and cycles; every even node carries
    the label L.  Returns (graph, typed edge list [(type, src, dst)], edge ids in list order)."""
    edges = []
    for _ in range(n_edges):
        s, d = int(rng.integers(0, n)), int(rng.integers(0, n))
        if acyclic:
            if s == d:
                d = (s + 1) % n
            s, d = min(s, d), max(s, d)
        edges.append((("KNOWS", "LIKES")[int(rng.integers(0, 2))], s, d))
    edges += [edges[0], edges[3]]
    return graph_of(n, edges, [("L", v) for v in range(0, n, 2)]), edges


def graph_of(n, typed_edges, labels=()):
    g = model.Graph(n)
    for name, v in labels:
        g.add_label(name)
        g.node_labels.add((v, g.label_ids[name]))
    pairs = {}
    for eid, (t, s, d) in enumerate(typed_edges):
        g.add_type(t)
        pairs.setdefault((g.type_ids[t], s, d), []).append(eid)
        g.adjacency.m.add((s, d))
    for (t, s, d), es in pairs.items():
        g.tensors[t].m[(s, d)] = es[0] if len(es) == 1 else model.MULTI_EDGE
        if len(es) > 1:
            g.tensors[t].me[(s, d)] = es
    return g
