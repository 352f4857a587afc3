#!/usr/bin/env python3
"""Generate tests/golden/sppaths_flow.json from the reference's tests/flow/test_path_algorithms.py.

usage: make_sppaths_golden.py <root of the reference tree>
Runs ONLY where the reference tree is present (like make_golden.py); the emitted JSON is committed, so pytest never reads the
reference.  Covered: the calls of that file that reach algo.SPpaths' single-path Dijkstra branch (pathCount 1, no maxLen, no
maxCost, source != target):
  test12  all three queries           test13  the five queries without maxLen
  test16  the pathCount 1 / no maxCost row            test17  part (a), the self-loop under relDirection 'both'
  test19 - test22  line, diamond, 4 x 4 grid and dense cyclic graphs: every ordered pair
What is read from the reference at run time:
  - the graphs of tests 12, 13, 16, 17: the CREATE statement of each method, parsed by the small pattern reader below;
  - the graphs of tests 19 - 22 and their expected weights: the four methods are compiled out of the file and run against a
    stand-in for `self` that records what they hand to the file's own verifier; the expected weight of every reachable pair is
    computed by the file's own all-pairs helper, compiled the same way.
The CALLS and ASSERTED VALUES of tests 12, 13, 16, 17 sit in query strings and assert statements; they are listed in CALLS below
with the lines they come from, and every literal listed is checked to occur in the method it is cited from."""
import ast
import heapq
import json
import os
import random
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FALKORDB_REFERENCE", "")
SRC = "tests/flow/test_path_algorithms.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sppaths_flow.json")

# (method, case name, config, expect, literals that must occur in the method, line)
CALLS = [
    ("test12_shortest_path_fast_path_results", "12_weighted_longer_route_is_cheaper",
     {"source": "A", "target": "C", "types": [], "direction": "outgoing", "weight": "weight", "cost": "cost"},
     {"found": True, "nodes": ["A", "B", "C"], "weight": 0.2, "delta": 1e-9, "cost": 2, "hops": 2}, ["A", "B", "C", 0.2, 2, 1e-9], "686-699"),
    ("test12_shortest_path_fast_path_results", "12_unweighted_direct_edge_wins",
     {"source": "A", "target": "C", "types": [], "direction": "outgoing", "weight": None, "cost": None},
     {"found": True, "nodes": ["A", "C"], "weight": 1, "delta": 0}, ["A", "C", 1], "702-707"),
    ("test12_shortest_path_fast_path_results", "12_unreachable_in_the_requested_direction",
     {"source": "C", "target": "A", "types": [], "direction": "outgoing", "weight": None, "cost": None},
     {"found": False}, [], "710-715"),
    ("test13_rel_direction_both", "13_A_C_outgoing",
     {"source": "A", "target": "C", "types": ["DR"], "direction": "outgoing", "weight": None, "cost": None},
     {"found": True, "hops": 2}, ["outgoing", 2], "736"),
    ("test13_rel_direction_both", "13_C_A_outgoing",
     {"source": "C", "target": "A", "types": ["DR"], "direction": "outgoing", "weight": None, "cost": None},
     {"found": False}, ["outgoing"], "737"),
    ("test13_rel_direction_both", "13_C_A_incoming",
     {"source": "C", "target": "A", "types": ["DR"], "direction": "incoming", "weight": None, "cost": None},
     {"found": True, "hops": 2}, ["incoming", 2], "738"),
    ("test13_rel_direction_both", "13_C_A_both",
     {"source": "C", "target": "A", "types": ["DR"], "direction": "both", "weight": None, "cost": None},
     {"found": True, "hops": 2}, ["both", 2], "739"),
    ("test13_rel_direction_both", "13_A_C_both",
     {"source": "A", "target": "C", "types": ["DR"], "direction": "both", "weight": None, "cost": None},
     {"found": True, "hops": 2}, ["both", 2], "740"),
    ("test16_sp_unreachable", "16_two_nodes_no_path",
     {"source": "X", "target": "Y", "types": [], "direction": "outgoing", "weight": "w", "cost": None},
     {"found": False}, [0], "818-819"),
    ("test17_sp_duplicate_edges", "17a_self_loop_under_both",
     {"source": "A", "target": "B", "types": [], "direction": "both", "weight": "weight", "cost": None},
     {"found": True, "weight": 1, "delta": 1e-9, "hops": 1}, [1, 1e-9], "840-854"),
]
GRAPH_TESTS = ["test19_dijkstra_line_graph", "test20_dijkstra_diamond_graph", "test21_dijkstra_grid_graph",
               "test22_dijkstra_dense_cyclic_graph"]


def methods():
    tree = ast.parse(open(os.path.join(REF, SRC)).read())
    out = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef):
            for f in cls.body:
                if isinstance(f, ast.FunctionDef):
                    out[f.name] = f
    return out


def constants(fn):
    """every literal of a method: the constants themselves and the words and numbers inside its strings"""
    found = set()
    for node in ast.walk(fn):
        if isinstance(node, ast.Constant):
            found.add(node.value)
            if isinstance(node.value, str):
                found.update(re.findall(r"[A-Za-z_]+", node.value))
                for num in re.findall(r"\d+(?:\.\d+)?(?:e-?\d+)?", node.value):
                    found.add(float(num) if ("." in num or "e" in num) else int(num))
    return found


def value(text):
    text = text.strip()
    if text[0] in "'\"":
        return text[1:-1]
    return float(text) if ("." in text or "e" in text) else int(text)


def props(text):
    if not text:
        return {}
    return {k.strip(): value(v) for k, v in (kv.split(":", 1) for kv in text.strip()[1:-1].split(","))}


def create_graph(fn):
    """nodes [[name, label]] and edges [[src, type, dst, attributes]] of the method's CREATE statement, in creation order"""
    stmt = next(c.value for c in ast.walk(fn) if isinstance(c, ast.Constant) and isinstance(c.value, str) and "CREATE" in c.value)
    var, nodes, edges = {}, [], []
    for m in re.finditer(r"\((\w+):(\w+)\s*(\{[^}]*\})?\)", stmt):
        name = props(m.group(3)).get("id", m.group(1))
        var[m.group(1)] = name
        nodes.append([name, m.group(2)])
    for m in re.finditer(r"\((\w+)\)-\[:(\w+)\s*(\{[^}]*\})?\]->\((\w+)\)", stmt):
        edges.append([var[m.group(1)], m.group(2), var[m.group(4)], props(m.group(3))])
    return nodes, edges


class Recorder:
    """stands in for `self` of the reference's test class: keeps what a test hands to the verifier"""

    def __init__(self, all_pairs):
        self.all_pairs = all_pairs
        self.seen = None

    def _verify_dijkstra_all_pairs(self, graph_name, n_nodes, edges):
        self.seen = (graph_name, n_nodes, [list(e) for e in edges])

    def _dijkstra_all_pairs(self, n_nodes, edges):
        return self.all_pairs(self, n_nodes, edges)


def compiled(fn):
    mod = ast.Module(body=[fn], type_ignores=[])
    ns = {"random": random, "heapq": heapq}
    exec(compile(mod, SRC, "exec"), ns)
    return ns[fn.name]


def main():
    assert os.path.isfile(os.path.join(REF, SRC)), __doc__.split("\n")[2]
    fns = methods()
    cases = []
    for method, name, config, expect, literals, line in CALLS:
        have = constants(fns[method])
        for lit in literals:
            assert lit in have, f"{method}: {lit!r} not found (cited from line {line})"
        nodes, edges = create_graph(fns[method])
        cases.append({"name": name, "line": f"{SRC}:{line}", "nodes": nodes, "edges": edges, "config": config, "expect": expect})
    all_pairs = compiled(fns["_dijkstra_all_pairs"])
    for method in GRAPH_TESTS:
        rec = Recorder(all_pairs)
        compiled(fns[method])(rec)
        graph, n, edges = rec.seen
        dist = rec._dijkstra_all_pairs(n, edges)
        pairs = [[s, t, dist[s].get(t)] for s in range(n) for t in range(n) if s != t]
        cases.append({"name": method[4:6] + "_" + graph, "line": f"{SRC}:{fns[method].lineno}-{fns[method].end_lineno}",
                      "nodes": [[str(i), "DK"] for i in range(n)],
                      "edges": [[str(u), "DE", str(v), {"weight": w}] for u, v, w in edges],
                      "config": {"types": [], "direction": "outgoing", "weight": "weight", "cost": None},
                      "expect": {"delta": 1e-9, "pairs": pairs}})
    doc = {
        "source": f"{SRC} of the reference: the graphs, calls and asserted results of its tests 12, 13 (without maxLen), 16 "
                  "(pathCount 1, no maxCost), 17 part (a) and 19 to 22; the expected weights of tests 19 to 22 are what the "
                  "file's own all-pairs Dijkstra helper returns for the graphs its test methods build",
        "format": "nodes: [name, label] in creation order (node id = index); edges: [src, type, dst, attributes] in creation "
                  "order (relationship id = index); config: source / target by node name, types = relTypes ([] = not given), "
                  "direction = relDirection, weight = weightProp, cost = costProp (null = not given); expect: found = whether "
                  "a row comes back, nodes = the asserted node names of the path, hops = its asserted length, weight = the "
                  "asserted pathWeight within delta (0 = equality), cost = the asserted pathCost; a case with expect.pairs "
                  "asks every ordered pair: [source, target, pathWeight within delta | null = no row]",
        "cases": cases,
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(OUT, len(cases), "cases")


if __name__ == "__main__":
    main()
