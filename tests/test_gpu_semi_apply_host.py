"""GPU: SemiApplyOp / OrApplyMultiplexerOp of the C++ host layer (semi_apply.rs:85-106, or_apply_multiplexer.rs:85-123) — the
passing rows against the rows that occur in oracle/model.py's expand_batch (matrix shapes) or expand_row / expand_into_row
(bidirectional, bound `to`), for semi and anti, and the three tiers against each other: the existence tier
(fgpu_expand_exists), the collect tier (device_exists = false, or a shape the existence tier does not take) and the per-row tier
(a shape no batch path takes).

Two graphs, each in the host layer and in the oracle model with the host's own (m, dp, dm) mirrored into the model: the multigraph
of test_gpu_expand_edges.random_graph (three types over shared pairs, multi-edges, self-loops, two labels) rebuilt through
create / commit / delete so that every tensor holds unfolded dp and dm, and test_gpu_host's R-MAT twin (build_random)."""
import os
import sys

import numpy as np
import pytest

from oracle import model
from falkordb_amd import host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_expand_edges import random_graph  # noqa: E402
from test_gpu_host import _twin_graphs, build_random, hctx  # noqa: E402,F401  (hctx: the host context fixture)

pytestmark = pytest.mark.gpu
NULL = "null"


def mirror(g, n, types, label_names, node_labels, final_ids):
    """The oracle model of a host graph, from the layers the host holds."""
    og = model.Graph(n)
    for name in label_names:
        og.add_label(name)
    og.node_labels |= set(node_labels)
    for t, name in enumerate(types):
        og.add_type(name)
        me = {p: sorted(es) for p, es in final_ids[t].items() if len(es) > 1}
        og.tensors[t] = model.Tensor(n, n, m={(r, c): v for r, c, v in g.layer(t, "m")},
                                     dp={(r, c): v for r, c, v in g.layer(t, "dp")},
                                     dm={(r, c) for r, c, _ in g.layer(t, "dm")}, me=me)
        for p, es in final_ids[t].items():
            assert og.tensors[t].get(*p) == sorted(es), (t, p)
    og.adjacency.m = {(r, c) for r, c, _ in g.layer(None, "m")}
    og.adjacency.dp.layer = {(r, c): True for r, c, _ in g.layer(None, "dp")}
    og.adjacency.dm.layer = {(r, c): True for r, c, _ in g.layer(None, "dm")}
    assert og.adjacency.extract() == set().union(*[set(f) for f in final_ids])
    return og


def layered_twin(hctx, seed=11, n=120, npairs=900):
    """random_graph's multigraph in the host layer, its final edges exactly.  What its tensors hold in m goes in first; its
    tombstoned pairs are then deleted, its shadowed pairs replaced and its dp pairs created — most of that committed as well,
    every sixth change left uncommitted (the fold policy empties a delta that is large beside its base), so that every tensor
    holds unfolded dp and dm."""
    rg = random_graph(seed, n, npairs)
    types = sorted(rg.type_ids, key=rg.type_ids.get)
    g = host.Graph(hctx, n)
    label_names = sorted(rg.label_ids, key=rg.label_ids.get)
    for name in label_names:
        lid = g.add_label(name)
        assert lid == rg.label_ids[name]
    for v, lid in sorted(rg.node_labels):
        g.label_node(v, lid)
    tids = [g.add_type(t) for t in types]
    first = []
    for t, ten in enumerate(rg.tensors):
        ids1 = {p: (list(ten.me[p]) if v == model.MULTI_EDGE else [v]) for p, v in ten.m.items()}
        first.append(ids1)
        for p, es in ids1.items():
            for e in es:
                g.create_edge(tids[t], p[0], p[1], e)
    g.commit()
    changed = [(t, p) for t, ten in enumerate(rg.tensors) for p in sorted(set(ten.m) | set(ten.dp))
               if sorted(first[t].get(p, [])) != sorted(ten.get(*p))]

    def apply(t, p):
        for e in first[t].get(p, []):
            g.delete_edge(tids[t], p[0], p[1], e)
        for e in rg.tensors[t].get(*p):
            g.create_edge(tids[t], p[0], p[1], e)

    for j, (t, p) in enumerate(changed):
        if j % 6:
            apply(t, p)
    g.commit()
    for j, (t, p) in enumerate(changed):
        if j % 6 == 0:
            apply(t, p)
    final = [{p: list(ten.get(*p)) for p in set(ten.m) | set(ten.dp) if ten.get(*p)} for ten in rg.tensors]
    og = mirror(g, n, types, label_names, rg.node_labels, final)
    for t in range(len(types)):
        sizes = [len(x) for x in (og.tensors[t].m, og.tensors[t].dp, og.tensors[t].dm, og.tensors[t].me)]
        assert all(sizes), sizes                                                    # unfolded deltas, multi-edges
    assert any(s == d for s, d in og.adjacency.extract())                          # self-loops
    return g, og, n


@pytest.fixture(scope="module")
def graphs(hctx):
    g1, og1, n1 = layered_twin(hctx)
    g2, og2, n2, _ = build_random(hctx)
    return {"layered": (g1, og1, n1, ["A", "B", "C"]), "rmat": (g2, og2, n2, ["A", "B"])}


def sources(n, k, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, k).tolist()
    src[3] = NULL                                   # bound to Null / a non-node: emits nothing
    src[k // 2] = NULL
    src[7] = src[6]                                 # the same source twice
    return src


def matrix_want(og, src, case):
    """The rows that occur in oracle.model.expand_batch over the node rows (a Null source emits nothing)."""
    idx = [i for i, v in enumerate(src) if v != NULL]
    res = model.expand_batch(og, [src[i] for i in idx], case["types"], src_labels=case.get("src", []),
                             dst_labels=case.get("dst", []), chain=case.get("chain", []))
    return sorted({idx[r[0]] for r in res[0]})


def row_want(og, src, to, case, transposed=False, bidir=False):
    out = []
    for i, f in enumerate(src):
        t = to[i] if to is not None else None
        if f == NULL or t == NULL:
            continue
        if model.expand_row(og, f, t, case["types"], from_labels=case.get("src", []), to_labels=case.get("dst", []),
                            transposed=transposed, bidirectional=bidir):
            out.append(i)
    return out


def both_ways(g, spec, src, to, want, k, tier, transposed=False, device_exists=True):
    """semi and anti under one setting: the passing rows, the tier that answered."""
    got, t, st = g.semi_apply(spec, src, to, transposed=transposed, device_exists=device_exists)
    assert got == want, (tier, sorted(set(got) ^ set(want))[:10])
    assert t == tier, (t, tier)
    anti, t2, _ = g.semi_apply(spec, src, to, anti=True, transposed=transposed, device_exists=device_exists)
    assert anti == [i for i in range(k) if i not in set(want)] and t2 == tier
    return st


MATRIX_CASES = [
    dict(types=["A"]),
    dict(types=[], src=["P"], dst=["Q"]),
    dict(types=["A", "B"], dst=["P"]),
    dict(types=["A"], src=["P"], chain=[(["B"], ["Q"])]),
    dict(types=[], chain=[([], []), (["A"], ["P"])]),
    dict(types=["B"], chain=[(["A"], []), (["B"], ["Q"])]),
    dict(types=["Nope"]),                                            # unknown type: no row matches
    dict(types=["A"], src=["NoSuchLabel"]),
    dict(types=["A"], dst=["NoSuchLabel"]),
    dict(types=["A", "Nope"]),
    dict(types=["A"], chain=[(["Nope", "B"], [])]),
]


def spec_of(case, **kw):
    hops = [(case["types"], case.get("dst", []))] + [tuple(h) for h in case.get("chain", [])]
    return host.cond_spec(src_labels=case.get("src", []), hops=hops, **kw)


@pytest.mark.parametrize("case", MATRIX_CASES, ids=lambda c: str(c)[:70])
@pytest.mark.parametrize("which", ["layered", "rmat"])
def test_matrix_shapes(graphs, which, case):
    g, og, n, _ = graphs[which]
    k = 200
    src = sources(n, k, 17)
    want = matrix_want(og, src, case)
    st = both_ways(g, spec_of(case), src, None, want, k, "exists")
    assert st[4] == (1 if want else st[4]) <= 1 and st[0] == len(want)     # one fgpu_expand_exists; its rows matched
    both_ways(g, spec_of(case), src, None, want, k, "collect", device_exists=False)
    if not case.get("chain"):
        assert want == row_want(og, src, None, case)
        both_ways(g, spec_of(case, attrs=True), src, None, want, k, "rows")      # inline attributes: no batch path takes it
    if case["types"] == ["A"] and len(case) == 1:
        assert 0 < len(want) < k - 2


@pytest.mark.parametrize("case", [dict(types=["B"]), dict(types=["A"], src=["Q"], dst=["P"]), dict(types=[], dst=["P"]),
                                  dict(types=["A", "B"], dst=["Q"]), dict(types=["Nope"])], ids=lambda c: str(c)[:70])
@pytest.mark.parametrize("which", ["layered", "rmat"])
def test_transposed(graphs, which, case):
    """The bound alias is the matrix destination: `WHERE ()-[:T]->(p)`."""
    g, og, n, _ = graphs[which]
    k = 120
    src = sources(n, k, 23)
    want = row_want(og, src, None, case, transposed=True)
    both_ways(g, spec_of(case), src, None, want, k, "exists", transposed=True)
    both_ways(g, spec_of(case), src, None, want, k, "collect", transposed=True, device_exists=False)
    both_ways(g, spec_of(case, attrs=True), src, None, want, k, "rows", transposed=True)


@pytest.mark.parametrize("transposed", [False, True], ids=["", "transposed"])
@pytest.mark.parametrize("case", [dict(types=["A"]), dict(types=[], src=["P"], dst=["Q"]), dict(types=["A", "B"], dst=["P"]),
                                  dict(types=["C", "Nope"]), dict(types=["Nope"])], ids=lambda c: str(c)[:70])
@pytest.mark.parametrize("which", ["layered", "rmat"])
def test_bidirectional(graphs, which, case, transposed):
    g, og, n, _ = graphs[which]
    k = 150
    src = sources(n, k, 29)
    want = row_want(og, src, None, case, transposed=transposed, bidir=True)
    st = both_ways(g, spec_of(case, bidir=True), src, None, want, k, "exists", transposed=transposed)
    known = [t for t in case["types"] if t in og.type_ids]
    assert st[4] == (2 if known or not case["types"] else 0)         # the forward and the transposed layers
    both_ways(g, spec_of(case, bidir=True), src, None, want, k, "collect", transposed=transposed, device_exists=False)
    both_ways(g, spec_of(case, bidir=True, attrs=True), src, None, want, k, "rows", transposed=transposed)
    # a relationship emitted, or sibling edges: the collect tier whatever device_exists says
    both_ways(g, spec_of(case, bidir=True, emit=True), src, None, want, k, "collect", transposed=transposed)
    both_ways(g, spec_of(case, emit=True), src, None, row_want(og, src, None, case, transposed=transposed), k, "collect",
              transposed=transposed)
    both_ways(g, spec_of(case, siblings=True), src, None, row_want(og, src, None, case, transposed=transposed), k, "collect",
              transposed=transposed)


@pytest.mark.parametrize("which", ["layered", "rmat"])
def test_bound_destination(graphs, which):
    """`WHERE NOT (a)-[:A]->(c)`: every row has `to` bound (the ExpandInto shape: the probe), then a mixed column."""
    g, og, n, _ = graphs[which]
    k = 160
    src = sources(n, k, 31)
    case = dict(types=["A"], dst=["P"])
    rng = np.random.default_rng(5)
    to = rng.integers(0, n, k).tolist()
    # half of the rows ask for a node the source really reaches
    reach = {}
    for (s, d) in og.tensors[og.type_ids["A"]].structure():
        reach.setdefault(s, []).append(d)
    for i in range(0, k, 2):
        if src[i] != NULL and reach.get(src[i]):
            to[i] = sorted(reach[src[i]])[len(reach[src[i]]) // 2]
    to[11] = NULL
    want = row_want(og, src, to, case)
    into = [i for i in range(k) if src[i] != NULL and to[i] != NULL
            and model.expand_into_row(og, src[i], to[i], ["A"], emit_relationship=False)
            and all(og.node_has_label_id(to[i], l) for l in og.resolve_label_ids(["P"]))]
    assert want == into and 0 < len(want) < k
    both_ways(g, spec_of(case), src, to, want, k, "exists")
    both_ways(g, spec_of(case), src, to, want, k, "collect", device_exists=False)
    both_ways(g, spec_of(case, attrs=True), src, to, want, k, "rows")
    # two hops, all bound
    chain = dict(types=["A"], chain=[([], [])])
    res = model.expand_batch(og, [s for s in src if s != NULL], ["A"], chain=[([], [])],
                             to_bound=[t if t != NULL else -1 for s, t in zip(src, to) if s != NULL])
    idx = [i for i, s in enumerate(src) if s != NULL]
    want2 = sorted({idx[r[0]] for r in res[0] if to[idx[r[0]]] != NULL})
    both_ways(g, spec_of(chain), src, to, want2, k, "exists")
    # a mixed column: some rows unbound — the collect tier
    mixed = [None if i % 3 == 0 else t for i, t in enumerate(to)]
    wantm = row_want(og, src, mixed, case)
    both_ways(g, spec_of(case), src, mixed, wantm, k, "collect")
    both_ways(g, spec_of(case, attrs=True), src, mixed, wantm, k, "rows")
    # bidirectional with `to` bound: the collect tier
    wantb = row_want(og, src, to, case, bidir=True)
    both_ways(g, spec_of(case, bidir=True), src, to, wantb, k, "collect")
    both_ways(g, spec_of(case, bidir=True, attrs=True), src, to, wantb, k, "rows")


def test_null_and_non_node_rows_cost_nothing(graphs):
    g, og, n, _ = graphs["layered"]
    src = [NULL] * 70
    got, tier, st = g.semi_apply(spec_of(dict(types=["A"])), src)
    assert got == [] and tier == "none" and st == [0, 0, 0, 0, 0]
    got, tier, _ = g.semi_apply(spec_of(dict(types=["A"])), src, anti=True)
    assert got == list(range(70)) and tier == "none"
    got, tier, st = g.semi_apply(spec_of(dict(types=["A"])), [1, 2, 3], [NULL, NULL, NULL])
    assert got == [] and tier == "none" and st[4] == 0
    assert g.semi_apply(spec_of(dict(types=["A"])), []) == ([], "none", [0, 0, 0, 0, 0])


def test_self_loops_and_small_twins(hctx):
    """A self-loop matches in either direction once; a node whose only edge comes in matches only bidirectionally."""
    edges = [("R", 0, 0), ("R", 1, 2), ("R", 1, 2), ("S", 3, 1), ("R", 4, 5)]
    for commit in (True, False):
        g, og = _twin_graphs(hctx, 8, edges, labels=[("P", 2), ("Q", 0)], commit=commit)
        src = [0, 1, 2, 3, 4, 5, 6, NULL]
        for case, bidir in ((dict(types=["R"]), False), (dict(types=["R"]), True), (dict(types=[], dst=["P"]), True),
                            (dict(types=["R", "S"]), True)):
            want = row_want(og, src, None, case, bidir=bidir)
            for de, tier in ((True, "exists"), (False, "collect")):
                both_ways(g, spec_of(case, bidir=bidir), src, None, want, 8, tier, device_exists=de)
            both_ways(g, spec_of(case, bidir=bidir, attrs=True), src, None, want, 8, "rows")
        assert row_want(og, src, None, dict(types=["R"]), bidir=True) == [0, 1, 2, 4, 5]
        assert row_want(og, src, None, dict(types=["R"])) == [0, 1, 4]


@pytest.mark.parametrize("device_exists", [True, False], ids=["exists", "collect"])
@pytest.mark.parametrize("which", ["layered", "rmat"])
def test_or_apply_multiplexer(graphs, which, device_exists):
    """`WHERE (p)-[:A]->(:P) OR NOT (p)-[:B]-() OR p.id % 5 = 0`, and with the anti flags the other way round: the union of the
    single-branch answers."""
    g, og, n, _ = graphs[which]
    k = 180
    src = sources(n, k, 37)
    s1, s2 = spec_of(dict(types=["A"], dst=["P"])), spec_of(dict(types=["B"]), bidir=True)
    col = [i % 5 == 0 for i in range(k)]
    for a1, a2, a3 in ((False, True, False), (True, False, True), (False, False, False)):
        one = set(g.semi_apply(s1, src, anti=a1, device_exists=device_exists)[0])
        two = set(g.semi_apply(s2, src, anti=a2, device_exists=device_exists)[0])
        three = {i for i in range(k) if col[i] != a3}
        got, tiers, stats = g.or_apply([(s1, a1), (s2, a2), (col, a3)], src, device_exists=device_exists)
        assert got == sorted(one | two | three)
        assert tiers == (["exists", "exists", "none"] if device_exists else ["collect", "collect", "none"])
        assert 0 < len(got) < k or (a1, a2, a3) != (False, False, False)
    # against the model, once
    w1 = set(matrix_want(og, src, dict(types=["A"], dst=["P"])))
    w2 = set(row_want(og, src, None, dict(types=["B"]), bidir=True))
    got, _, _ = g.or_apply([(s1, False), (s2, True), (col, False)], src, device_exists=device_exists)
    assert got == sorted(w1 | (set(range(k)) - w2) | {i for i in range(k) if col[i]})
