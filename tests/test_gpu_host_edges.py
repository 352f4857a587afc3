"""CondTraverseOp::expand_batch_edges (host layer over ONE fgpu_expand_edges) through fh_cond_traverse_edges_batch: equal to
oracle.model.expand_row row by row and to the existing per-row path cond_traverse_rows on the same graph, declined where the
issue keeps the per-row path, and never served from a stale multi-edge table."""
import itertools

import numpy as np
import pytest

from falkordb_amd import host
from oracle import model

pytestmark = pytest.mark.gpu
MULTI = model.MULTI_EDGE
N = 200
TYPES = ["A", "B", "C"]


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def oracle_of(n, per_type, labels):
    """the oracle graph of a pair model: per_type[t] = {(src, dst): [edge ids]} (expand_row reads the effective state only)"""
    og = model.Graph(n)
    for name, nodes in labels.items():
        lid = og.add_label(name)
        og.node_labels |= {(v, lid) for v in nodes}
    for t, pairs in enumerate(per_type):
        og.add_type(TYPES[t])
        og.tensors[t] = model.Tensor(n, n, m={p: (es[0] if len(es) == 1 else MULTI) for p, es in pairs.items()},
                                     me={p: sorted(es) for p, es in pairs.items() if len(es) > 1})
    og.adjacency.m = set().union(*[set(p) for p in per_type])
    return og


class Twin:
    """200 nodes, 3 types over shared pairs, multi-edges and self-loops; a committed transaction and an uncommitted one on top
    (promotions, fresh pairs, deletions): every layer of every tensor holds something"""

    def __init__(self, hctx, seed=7, commit_all=False):
        rng = np.random.default_rng(seed)
        self.g = host.Graph(hctx, N)
        self.labels = {"P": [v for v in range(N) if v % 3 == 0], "Q": [v for v in range(N) if v % 2 == 1]}
        for name, nodes in self.labels.items():
            lid = self.g.add_label(name)
            for v in nodes:
                self.g.label_node(v, lid)
        self.tids = [self.g.add_type(t) for t in TYPES]
        self.per_type = [{}, {}, {}]
        self.eid = 0
        cand = [(int(a), int(b)) for a, b in rng.integers(0, N, (700, 2))] + [(int(v), int(v)) for v in rng.integers(0, N, 12)]
        for t in range(3):
            sel = [cand[j] for j in rng.choice(len(cand), 420, replace=True)]   # with repetition: multi-edge pairs
            self.create(t, sel, bulk=True)
        self.g.commit()
        for t in range(3):
            keys = sorted(self.per_type[t])
            self.create(t, [keys[j] for j in rng.choice(len(keys), 40, replace=False)])          # promotions
            self.create(t, [(int(a), int(b)) for a, b in rng.integers(0, N, (40, 2))])           # fresh pairs
            for j in rng.choice(len(keys), 50, replace=False):                                  # deletions
                for e in self.per_type[t].pop(keys[j], []):
                    self.g.delete_edge(self.tids[t], keys[j][0], keys[j][1], e)
        if commit_all:
            self.g.commit()

    def create(self, t, pairs, bulk=False):
        ids = list(range(self.eid, self.eid + len(pairs)))
        self.eid += len(pairs)
        if bulk:
            self.g.create_edges(self.tids[t], [p[0] for p in pairs], [p[1] for p in pairs], ids)
        for p, e in zip(pairs, ids):
            if not bulk:
                self.g.create_edge(self.tids[t], p[0], p[1], e)
            self.per_type[t].setdefault(p, []).append(e)
        return ids

    def oracle(self):
        return oracle_of(N, self.per_type, self.labels)


@pytest.fixture(scope="module")
def twin(hctx):
    t = Twin(hctx)
    st = t.g.tensor_state(t.tids[0])
    assert st["dp"] > 0 and st["dm"] > 0 and st["multi_pairs"] > 0               # the layers really are dirty
    return t, t.oracle()


def batch_rows(tw):
    rng = np.random.default_rng(3)
    pairs = sorted(set().union(*[set(p) for p in tw.per_type]))
    sel = [pairs[j] for j in rng.choice(len(pairs), 30, replace=False)]
    rows = [(p[0], None) for p in sel[:12]] + [(None, p[1]) for p in sel[12:22]] + sel[22:] + [(p[1], p[0]) for p in sel[:4]]
    rows += [(int(v), None) for v in rng.integers(0, N, 6)] + [("x", None), (5, "x"), (sel[0][0], None), (sel[0][0], None)]
    return rows


def want(og, rows, types, used=None, **kw):
    out, hit, memo = [], set(), {}
    for i, (f, t) in enumerate(rows):
        if isinstance(f, str) or isinstance(t, str):
            continue
        key = (f, t, id(used[i]) if used else 0)                                # (the rows of a batch repeat)
        if key not in memo:
            memo[key] = model.expand_row(og, f, t, types, used_edges=used[i] if used else (), **kw)
        for x in memo[key]:
            out.append((i,) + x)
            hit.add(i)
    return out, [i for i in range(len(rows)) if i not in hit]


LABELS = [dict(), dict(from_labels=["P"]), dict(to_labels=["Q"]), dict(from_labels=["Q"], to_labels=["P"]),
          dict(from_labels=["NoSuchLabel"])]


@pytest.mark.parametrize("emit,bidir,transposed", list(itertools.product([True, False], repeat=3)))
def test_batch_matches_the_oracle(twin, emit, bidir, transposed):
    tw, og = twin
    rows = batch_rows(tw)
    rng = np.random.default_rng(17)
    all_ids = [e for pt in tw.per_type for es in pt.values() for e in es]
    lists = [sorted(int(x) for x in rng.choice(all_ids, 300 + j, replace=False)) for j in range(3)]   # of differing lengths
    used = [lists[i % 3] for i in range(len(rows))]
    f, t = [r[0] for r in rows], [r[1] for r in rows]
    for siblings, optional, lab, types in itertools.product([False, True], [False, True], LABELS, (["A"], ["C", "A", "B"], [])):
        if lab and types == [] and optional:
            continue                                                            # (keeps the case count down; covered below)
        spec = host.cond_spec(src_labels=lab.get("from_labels", []), hops=[(types, lab.get("to_labels", []))], emit=emit,
                              bidir=bidir, siblings=siblings, optional=optional)
        res = tw.g.cond_traverse_edges_batch(spec, f, t, transposed=transposed, used_edges=used if siblings else None)
        if not (emit or bidir or siblings):
            assert res is None                                                  # the matrix path's pattern: declined
            continue
        got, nulls, st = res
        w, wn = want(og, rows, types, used if siblings else None, transposed=transposed, bidirectional=bidir,
                     emit_relationship=emit, **lab)
        assert got == w, (spec, [x for x in zip(got, w) if x[0] != x[1]][:3])
        assert nulls == (wn if optional else [])


def test_full_matrix_rows_are_spliced_in(twin):
    tw, og = twin
    rows = [(3, None), (None, None), (None, 9), (None, None), (9, None)]
    for emit, bidir in ((True, False), (False, True)):
        spec = host.cond_spec(hops=[(["B", "A"], [])], emit=emit, bidir=bidir)
        got, nulls, _ = tw.g.cond_traverse_edges_batch(spec, [r[0] for r in rows], [r[1] for r in rows])
        assert got == want(og, rows, ["B", "A"], emit_relationship=emit, bidirectional=bidir)[0]
        assert len([r for r in got if r[0] == 1]) > 300


@pytest.mark.parametrize("case", [dict(types=["A"], emit=True), dict(types=["C", "A"], emit=True, bidir=True),
                                  dict(types=[], emit=False, bidir=True, from_labels=["P"]),
                                  dict(types=["B"], emit=True, transposed=True, to_labels=["Q"]),
                                  dict(types=["A", "B"], emit=False, siblings=True),
                                  dict(types=["Nope"], emit=True), dict(types=["A", "Nope"], emit=True),
                                  dict(types=["Nope", "A"], emit=True),                  # the unknown name first
                                  dict(types=["A", "A"], emit=True),                     # a name listed twice stays twice
                                  dict(types=["A", "A"], emit=False, bidir=True),
                                  dict(types=["Nope", "Nada"], emit=True, optional=True)], ids=str)
def test_batch_equals_the_per_row_path(twin, case):
    tw, og = twin
    rows = batch_rows(tw)[:40] + [("x", None)]
    f, t = [r[0] for r in rows], [r[1] for r in rows]
    used = sorted(e for pt in tw.per_type for es in list(pt.values())[::3] for e in es[:1]) if case.get("siblings") else []
    spec = host.cond_spec(src_labels=case.get("from_labels", []), hops=[(case["types"], case.get("to_labels", []))],
                          emit=case["emit"], bidir=case.get("bidir", False), siblings=case.get("siblings", False),
                          optional=case.get("optional", False))
    tr = case.get("transposed", False)
    got, nulls, _ = tw.g.cond_traverse_edges_batch(spec, f, t, transposed=tr, used_edges=[used] * len(rows) if used else None)
    assert got == tw.g.cond_traverse_rows(spec, f, t, transposed=tr, used_edges=used)
    if case["types"] == ["A", "A"] and case["emit"]:
        single = host.cond_spec(hops=[(["A"], [])], emit=True)
        assert sorted(got) == sorted(2 * tw.g.cond_traverse_rows(single, f, t))           # every id of A, twice
    if case.get("optional"):
        assert got == [] and nulls == list(range(len(rows)))                             # no known type: every row null-pads
    elif "Nope" not in case["types"]:
        assert len(got) > 20


def test_declined_batches_run_nothing(twin):
    tw, _ = twin
    L = host.load()
    fused = host.cond_spec(hops=[(["A"], []), (["B"], [])])
    assert L.fh_cond_traverse_eligible(fused) == 1
    assert tw.g.cond_traverse_edges_batch(fused, [1, 2], [None, None]) is None                  # a fused chain
    bid = host.cond_spec(hops=[([], [])], emit=False, bidir=True)
    assert tw.g.cond_traverse_edges_batch(bid, [1, 2], [None, None], dedup=True) is None        # the cross-row dedup
    assert tw.g.cond_traverse_edges_batch(bid, [1, 2], [None, None]) is not None
    assert tw.g.cond_traverse_edges_batch(host.cond_spec(hops=[(["A"], [])], emit=True, attrs=True), [1], [None]) is None
    assert L.fh_cond_traverse_eligible(bid) == 0                                                # the reference's rule stands


def test_every_mutation_drops_the_cached_table(hctx):
    """after append_edges_bulk, delete_edges_bulk, delete_nodes_bulk and a plain create_edges the next batch emits the new
    ids; a version dup()ed before keeps answering from its own state"""
    tw = Twin(hctx, seed=9, commit_all=True)
    g = tw.g
    spec = host.cond_spec(hops=[(["A", "B", "C"], [])], emit=True, bidir=True)
    nodes = list(range(N))

    def agree():
        got, _, st = g.cond_traverse_edges_batch(spec, nodes, [None] * N)
        assert got == want(tw.oracle(), [(v, None) for v in nodes], ["A", "B", "C"], emit_relationship=True, bidirectional=True)[0]
        return st

    assert agree()[3] > 0                                                        # multi-edge pairs expanded: the table is built
    multi = [p for p, es in sorted(tw.per_type[0].items()) if len(es) > 1]
    single = [p for p, es in sorted(tw.per_type[0].items()) if len(es) == 1]
    old = g.tensor_version(tw.tids[0])
    old_ids = old.get(*multi[0])
    # append: a multi-edge pair grows, a single pair is promoted, a new pair arrives
    batch = [multi[0], multi[0], single[0], (199, 198)]
    ids = list(range(tw.eid, tw.eid + 4))
    tw.eid += 4
    g.append_edges_bulk(tw.tids[0], [p[0] for p in batch], [p[1] for p in batch], ids)
    for p, e in zip(batch, ids):
        tw.per_type[0].setdefault(p, []).append(e)
    agree()
    assert old.get(*multi[0]) == old_ids and g.tensor_get(tw.tids[0], *multi[0]) == old_ids + ids[:2]
    # delete edges: a multi-edge pair shrinks, another is demoted
    kill = [(multi[0], tw.per_type[0][multi[0]][0])] + [(multi[1], e) for e in tw.per_type[0][multi[1]][1:]]
    g.delete_edges_bulk(tw.tids[0], [p[0] for p, _ in kill], [p[1] for p, _ in kill], [e for _, e in kill])
    for p, e in kill:
        tw.per_type[0][p].remove(e)
    agree()
    # detach two nodes
    gone = {multi[2][0], multi[3][1]}
    g.delete_nodes_bulk(sorted(gone))
    for pt in tw.per_type:
        for p in [p for p in pt if p[0] in gone or p[1] in gone]:
            del pt[p]
    agree()
    # a plain create_edges promotes a pair
    keep = next(p for p in single[1:] if p in tw.per_type[0])
    tw.create(0, [keep, keep], bulk=True)
    agree()
    g.commit()
    agree()
