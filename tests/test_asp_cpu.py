"""CPU: the two checkers of tests/asp_check.py (what the GPU tests hold fgpu_shortest_dag and Graph.all_shortest_paths to)
against the reference's own graphs and asserted results (tests/golden/asp_flow.json, written by tests/golden/make_asp_golden.py)
and against each other: the pairs the operator's paths traverse are the shortest-path DAG, and there are as many paths as the
DAG has walks."""
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asp_check import path_count, pairs_of_paths, pattern, random_multigraph, reference_paths, shortest_dag  # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asp_flow.json")))


def edges_of(graph):
    return [(i, t, s, d) for i, (s, t, d) in enumerate(GOLD["graphs"][graph]["edges"])]


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_reference_paths_reproduces_the_asserted_results(case):
    g = GOLD["graphs"][case["graph"]]
    paths = reference_paths(len(g["nodes"]), edges_of(case["graph"]), case["src"], case["dst"], case["types"],
                            case["bidirectional"], case["reversed"], case["max_hops"])
    assert sorted(sorted(p) for p in paths) == case["expect_id_sets"]
    assert all(len(set(p)) == len(p) for p in paths)


def test_the_golden_file_lists_what_it_leaves_out():
    text = " ".join(GOLD["not_covered"])
    assert "test03" in text and "test04" in text


def hold_dag_to_paths(n, edges, src, dst, types, bidirectional, reversed):
    """every max_hops of {unbounded, L, L - 1, 0}: the DAG of the pattern is what the operator's paths traverse"""
    rows, cols, mult = pattern(edges, types, bidirectional)
    L, _ = shortest_dag(n, rows, cols, src, dst, -1)
    seen = 0
    for mh in {None, L, L - 1, 0} if L > 0 else {None, 0, 3}:
        paths = reference_paths(n, edges, src, dst, types, bidirectional, reversed, mh)
        Lm, pairs = shortest_dag(n, rows, cols, src, dst, -1 if mh is None else mh)
        if mh is None or mh >= L > 0:
            assert Lm == L
        else:
            assert Lm == -1 and pairs == []
        if Lm < 0:
            assert paths == []
            continue
        assert all(len(p) == Lm for p in paths)
        assert pairs_of_paths(paths, edges, bidirectional, src, src == dst, reversed) == [(u, v) for u, v, _ in pairs]
        assert all(0 <= d < Lm for _, _, d in pairs)
        assert len(paths) == path_count(Lm, pairs, src, dst, mult) > 0
        assert len(set(map(tuple, paths))) == len(paths)
        seen += 1
    return seen


@pytest.mark.parametrize("graph", ["acyclic", "cyclic", "acyclic_07"])
def test_dag_equals_the_pairs_of_the_paths_on_the_golden_graphs(graph):
    n, edges = len(GOLD["graphs"][graph]["nodes"]), edges_of(graph)
    found = 0
    for bidirectional in (False, True):
        for types in ([], ["E"], ["E2", "E"]):
            for s in range(n):
                for d in range(n):
                    found += hold_dag_to_paths(n, edges, s, d, types, bidirectional, reversed=(s + d) % 2 == 1)
    assert found > 20


def test_dag_equals_the_pairs_of_the_paths_on_random_multigraphs():
    found = cycles = 0
    for seed in range(200):
        rng = random.Random(0xA5F0 + seed)
        n = rng.randint(2, 12)
        edges = random_multigraph(rng, n, rng.randint(1, 3 * n), ["A", "B", "C"])
        bidirectional = seed % 2 == 1
        types = [[], ["B", "A"], ["C"]][seed % 3]
        for k in range(6):
            s = rng.randrange(n)
            d = s if k < 2 else rng.randrange(n)
            got = hold_dag_to_paths(n, edges, s, d, types, bidirectional, reversed=rng.random() < 0.5)
            found += got
            cycles += got if s == d else 0
    assert found > 500 and cycles > 100
