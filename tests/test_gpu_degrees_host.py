"""indegree() / outdegree() through the host layer (host.Graph.node_degrees, DegreeFn): the batch — ONE fgpu_node_degrees call —
equals the per-row host loop and the oracle, before and after commit; the reference's type resolution; the social fixture with
the reference's test27_edge_counting (tests/flow/test_social.py:337-355) restated over the traversal's own rows."""
import gc
import json
import os
from collections import Counter

import numpy as np
import pytest

from falkordb_amd import host

from oracle import model

pytestmark = pytest.mark.gpu
MULTI = model.MULTI_EDGE
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def hctx():
    c = host.Context(0)
    yield c
    c.close()


def oracle_graph(n, names, per_type):
    og = model.Graph(n)
    for t, name in enumerate(names):
        og.add_type(name)
        og.tensors[t] = model.Tensor(n, n, m={p: (es[0] if len(es) == 1 else MULTI) for p, es in per_type[t].items()},
                                     me={p: es for p, es in per_type[t].items() if len(es) > 1})
    og.adjacency.m = set().union(*[set(p) for p in per_type])
    return og


def counts(per_type, tids):
    """one pass over the live relationships of the types `tids`: (out, in) Counters"""
    o, i = Counter(), Counter()
    for t in tids:
        for (s, d), es in per_type[t].items():
            o[s] += len(es)
            i[d] += len(es)
    return o, i


def hold(g, og, per_type, names, n, sample):
    """batch == per row == the one-pass count, for out and in, over several type lists; the oracle on a sample of nodes"""
    nodes = list(range(n)) + [n - 1, 0, 0]
    for types in ((), ("Y",), ("Z", "X"), ("X", "X"), ("nope", "Y"), ("nope",), ("nope", "neither")):
        known = list(dict.fromkeys(t for t in types if t in names))
        tids = [names.index(t) for t in known] if types else list(range(len(names)))
        want_o, want_i = counts(per_type, tids)
        for incoming, want in ((False, want_o), (True, want_i)):
            got, st = g.node_degrees(nodes, incoming=incoming, types=types, stats=True)
            assert got.tolist() == [want[v] for v in nodes], (types, incoming)
            assert st["device_calls"] == (1 if tids else 0)
            rows = g.node_degrees(nodes, incoming=incoming, types=types, batched=False)
            assert rows.tolist() == got.tolist()
            if types and not tids:
                continue                                   # (the oracle reads a list of unknown names as "every tensor" too)
            for v in sample:
                # the oracle keeps a name listed twice; the function counts it once: ask it for the distinct names
                assert len(model.node_relationships(og, v, known, not incoming, incoming)) == want[v]
        alln = g.node_degrees_all(incoming=False, types=types)
        assert alln.tolist() == [want_o[v] for v in range(n)]
    assert g.node_degrees([], incoming=True).tolist() == []


def test_random_multigraph_before_and_after_commit(hctx):
    n, names = 70, ["X", "Y", "Z"]
    rng = np.random.default_rng(17)
    g = host.Graph(hctx, n)
    per_type, eid = [{}, {}, {}], 0
    tids = [g.add_type(name) for name in names]
    for t in range(3):
        for round_ in range(2):
            s, d = rng.integers(0, n, 150).tolist(), rng.integers(0, n, 150).tolist()
            s[:6], d[:6] = [5, 5, 5, 9, 9, 12], [5, 5, 6, 9, 3, 12]     # self-loops, inline and multi-edge
            for a, b in zip(s, d):
                g.create_edge(tids[t], a, b, eid)
                per_type[t].setdefault((a, b), []).append(eid)
                eid += 1
            if round_ == 0:
                g.commit()                                               # the second round stays pending: dp
        for p in list(per_type[t])[:20]:                                 # pending deletions: dm, and lists that shrink
            es = per_type[t][p]
            for e in (es if len(es) == 1 or p[0] % 2 else es[:1]):
                g.delete_edge(tids[t], p[0], p[1], e)
            left = [e for e in es if e not in (es if len(es) == 1 or p[0] % 2 else es[:1])]
            if left:
                per_type[t][p] = left
            else:
                del per_type[t][p]
    og = oracle_graph(n, names, per_type)
    sample = [5, 9, 12, 3, 6] + list(range(20, 35))
    hold(g, og, per_type, names, n, sample)
    g.commit()
    hold(g, og, per_type, names, n, sample)
    # an id at the capacity is an error in both paths, before any result
    for batched in (True, False):
        with pytest.raises(host.HostError) as e:
            g.node_degrees([1, n], batched=batched)
        assert "capacity" in str(e.value)
    # DETACH DELETE: once committed, the node's rows are empty and it answers 0 (tests/flow/test_results.py:226-234)
    victim = 5
    assert g.node_degrees([victim])[0] > 0 and g.node_degrees([victim], incoming=True)[0] > 0
    g.delete_nodes_bulk([victim])
    g.commit()
    for t in range(3):
        per_type[t] = {p: es for p, es in per_type[t].items() if victim not in p}
    for batched in (True, False):
        assert g.node_degrees([victim, victim], batched=batched).tolist() == [0, 0]
        assert g.node_degrees([victim], incoming=True, batched=batched).tolist() == [0]
    hold(g, oracle_graph(n, names, per_type), per_type, names, n, sample)
    del g
    gc.collect()


def social(hctx, commit):
    """tests/golden/social.json as tests/test_gpu_host.py builds it"""
    with open(os.path.join(GOLD, "social.json")) as f:
        s = json.load(f)
    names = [p["name"] for p in s["persons"]] + s["countries"]
    ids = {n: i for i, n in enumerate(names)}
    g = host.Graph(hctx, len(names))
    lp, lc = g.add_label("person"), g.add_label("country")
    for p in s["persons"]:
        g.label_node(ids[p["name"]], lp)
    for c in s["countries"]:
        g.label_node(ids[c], lc)
    tf, tv = g.add_type("friend"), g.add_type("visited")
    eid = 0
    for a, b, _purpose in s["visits"]:
        g.create_edge(tv, ids[a], ids[b], eid)
        eid += 1
    if commit:
        g.commit()
    for a, b in s["friends"]:
        g.create_edge(tf, ids[a], ids[b], eid)
        eid += 1
    if commit:
        g.commit()
    return s, g, ids, names


@pytest.mark.parametrize("commit", [False, True], ids=["pending-deltas", "committed"])
def test_social_edge_counting(hctx, commit):
    """test27_edge_counting: outdegree(a) equals the per-node count of (a)-[e]->(b), for every person; the same for indegree
    and for both with the type named"""
    s, g, ids, names = social(hctx, commit)
    persons = [ids[p["name"]] for p in s["persons"]]
    k = len(persons)
    assert sum(len(v) for v in (s["visits"], s["friends"])) > 0
    for types in ((), ("friend",)):
        spec = host.cond_spec(hops=[(list(types), [])], emit=True)
        for incoming in (False, True):
            froms, tos = ([None] * k, persons) if incoming else (persons, [None] * k)
            cols, _, _ = g.cond_traverse_edges_batch(spec, froms, tos, as_arrays=True)
            want = np.bincount(cols[0].astype(np.int64), minlength=k)
            got, st = g.node_degrees(persons, incoming=incoming, types=types, stats=True)
            assert got.tolist() == want.tolist() and st["device_calls"] == 1
            assert g.node_degrees(persons, incoming=incoming, types=types, batched=False).tolist() == want.tolist()
            everyone = g.node_degrees_all(incoming=incoming, types=types)
            assert everyone.tolist() == g.node_degrees(np.arange(len(names)), incoming=incoming, types=types).tolist()
            assert everyone[persons].tolist() == want.tolist()
    # the reference's query: the persons with outdegree(a) > 0 are those the pattern (a)-[e]->(b) matches at all
    out = g.node_degrees(persons)
    sources = {ids[a] for a, _b, _p in s["visits"]} | {ids[a] for a, _b in s["friends"]}
    assert {persons[j] for j in range(k) if out[j] > 0} == sources & set(persons)
    assert int(out.sum()) == sum(1 for a, _b, _p in s["visits"] if ids[a] in set(persons)) + \
        sum(1 for a, _b in s["friends"] if ids[a] in set(persons))
    del g
    gc.collect()
