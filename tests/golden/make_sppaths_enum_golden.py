#!/usr/bin/env python3
"""Generate tests/golden/sppaths_enum_flow.json from the reference's tests/flow/test_path_algorithms.py.

usage: make_sppaths_enum_golden.py <root of the reference tree>
Runs ONLY where the reference tree is present (like make_sppaths_golden.py, whose readers it shares); the emitted JSON is
committed, so pytest never reads the reference.  Covered: the calls of that file that LEAVE algo.SPpaths' single-path Dijkstra
branch (pathCount 0 or > 1, maxLen, maxCost) and its algo.SSpaths call on a fixed graph:
  test08  both procedures                       test09  the four enumeration shapes (the first one is the fast shape)
  test10  the six rows with maxLen              test11  both graphs, the five shapes that are not the fast one, and the sibling graph
  test16  the three rows with maxCost
Tests 02 to 07, 15, 17 (b) and 18 run on a graph built with rand() and cannot be fixtures; 17 (a) is the fast shape
(sppaths_flow.json has it).
What is read from the reference at run time:
  - the graphs of tests 08, 11, 16: the CREATE statements of each method, parsed by make_sppaths_golden.py's pattern reader;
  - the graphs of tests 09 and 10: _populate_branchy_graph's rule y = 1 + (x * 7919 + k * 104729) % blob for x in 1 .. blob, k in
    1 .. fanout, plus the node v = 0 nothing points at — the multipliers and the statement's shape are checked to occur in that
    method, blob and fanout in the calling test; the pairs are emitted in creation order (x-major), node v >= 1 is node id
    v - 1 and v = 0 is node id blob (the order the statements create them in).
The CALLS and ASSERTED VALUES sit in query strings and assert statements; they are listed in CALLS below with the lines they come
from, and every literal listed is checked to occur in the method it is cited from."""
import ast
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_sppaths_golden import REF, SRC, constants, methods, props  # noqa: E402

import re  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sppaths_enum_flow.json")


def call(proc, source, target, expect, types=(), direction="outgoing", weight=None, cost=None, max_len=None, max_cost=None,
         path_count=1):
    return {"proc": proc, "source": source, "target": target, "types": list(types), "direction": direction, "weight": weight,
            "cost": cost, "max_len": max_len, "max_cost": max_cost, "path_count": path_count, "expect": expect}


# (method, case name, graph: ("create", index of the CREATE statement) | ("branchy", blob, fanout), call, literals, lines)
CALLS = [
    ("test08_fractional_weights", "08_sp_two_paths_ordered_by_fractional_weight", ("create", 0),
     call("sp", "A", "C", {"rows": 2, "weights_desc": [0.9, 0.2], "delta": 1e-9}, weight="weight", max_len=3, path_count=2),
     ["A", "C", "weight", "maxLen", 3, "pathCount", 2, 0.9, 0.2, 1e-9, "SPpaths"], "485-503"),
    ("test08_fractional_weights", "08_ss_two_lightest_of_three", ("create", 0),
     call("ss", "A", None, {"rows": 2, "weights_desc": [0.2, 0.1], "delta": 1e-9}, weight="weight", max_len=3, path_count=2),
     ["A", "weight", "maxLen", 3, "pathCount", 2, 0.2, 0.1, 1e-9, "SSpaths"], "510-525"),
]
for _name, _extra, _lits in (("maxLen_12", {"max_len": 12}, ["maxLen", 12]), ("pathCount_0", {"path_count": 0}, ["pathCount", 0]),
                             ("pathCount_4", {"path_count": 4}, ["pathCount", 4]),
                             ("maxCost_500", {"max_cost": 500, "cost": "nonexistent"}, ["maxCost", 500, "costProp", "nonexistent"])):
    CALLS.append(("test09_unreachable_target_terminates", "09_unreachable_" + _name, ("branchy", 200, 8),
                  call("sp", 1, 0, {"rows": 0}, types=["BE"], **_extra), ["BE", "outgoing", 200, 8] + _lits, "563-575"))
for _s, _t, _extra, _want, _line in ((1, 137, {"max_len": 6}, [6], "604"), (42, 299, {"max_len": 6}, [5], "605"),
                                     (7, 88, {"max_len": 6}, [4], "606"), (7, 88, {"max_len": 5, "path_count": 0}, [4, 4], "609"),
                                     (7, 88, {"max_len": 6, "path_count": 3}, [4, 4, 6], "610"),
                                     (1, 137, {"max_len": 5, "path_count": 0}, [], "612")):
    CALLS.append(("test10_deep_search_results",
                  f"10_deep_{_s}_{_t}_maxLen_{_extra['max_len']}_pathCount_{_extra.get('path_count', 1)}", ("branchy", 3000, 8),
                  call("sp", _s, _t, {"rows": len(_want), "lengths_sorted": _want}, types=["BE"], **_extra),
                  ["BE", "outgoing", 3000, 8, _s, _t, "maxLen", _extra["max_len"]] + _want
                  + (["pathCount", _extra["path_count"]] if "path_count" in _extra else []), _line))
for _name, _extra, _lits in (("maxLen_10", {"max_len": 10}, ["maxLen", 10]), ("maxLen_3", {"max_len": 3}, ["maxLen", 3]),
                             ("pathCount_0_maxLen_10", {"path_count": 0, "max_len": 10}, ["pathCount", 0, "maxLen", 10]),
                             ("pathCount_2_maxLen_10", {"path_count": 2, "max_len": 10}, ["pathCount", 2, "maxLen", 10]),
                             ("maxCost_100_costProp_weight", {"max_cost": 100, "cost": "weight"}, ["maxCost", 100, "costProp"])):
    CALLS.append(("test11_fractional_weights_through_enumeration", "11_frac_enum_" + _name, ("create", 0),
                  call("sp", "A", "D", {"rows": 1, "weights_desc": [0.6], "delta": 1e-9}, weight="weight", **_extra),
                  ["A", "D", "weight", 0.6, 1e-9, 1] + _lits, "633-648"))
CALLS.append(("test11_fractional_weights_through_enumeration", "11_frac_sibling_maxLen_10", ("create", 1),
              call("sp", "S", "T", {"rows": 1, "weights_desc": [0.6], "delta": 1e-9}, weight="weight", max_len=10),
              ["S", "T", "weight", "maxLen", 10, 0.6, 1e-9, 1], "662-669"))
for _pc, _line in ((1, "821"), (0, "823"), (3, "825")):
    CALLS.append(("test16_sp_unreachable", f"16_two_nodes_no_path_pathCount_{_pc}_maxCost_100", ("create", 0),
                  call("sp", "X", "Y", {"rows": 0}, weight="w", max_cost=100, path_count=_pc), ["X", "Y", "w", "maxCost", 100, _pc, 0],
                  _line))


def create_graphs(fn):
    """per CREATE statement of the method, in source order: nodes [[name, label]] and edges [[src, type, dst, attributes]] in
    creation order (make_sppaths_golden.create_graph for every statement instead of the first)"""
    stmts = sorted((c.lineno, c.value) for c in ast.walk(fn)
                   if isinstance(c, ast.Constant) and isinstance(c.value, str) and "CREATE" in c.value and "UNWIND" not in c.value)
    out = []
    for _, stmt in stmts:
        var, nodes, edges = {}, [], []
        for m in re.finditer(r"\((\w+):(\w+)\s*(\{[^}]*\})?\)", stmt):
            name = props(m.group(3)).get("id", m.group(1))
            var[m.group(1)] = name
            nodes.append([name, m.group(2)])
        for m in re.finditer(r"\((\w+)\)-\[:(\w+)\s*(\{[^}]*\})?\]->\((\w+)\)", stmt):
            edges.append([var[m.group(1)], m.group(2), var[m.group(4)], props(m.group(3))])
        out.append((nodes, edges))
    return out


def branchy(fns, blob, fanout):
    have = constants(fns["_populate_branchy_graph"])
    for lit in (7919, 104729, "UNWIND", "range", "BE", "B", "v", 0, 1):
        assert lit in have, f"_populate_branchy_graph: {lit!r} not found (cited from lines 527-543)"
    dst = [1 + (x * 7919 + k * 104729) % blob for x in range(1, blob + 1) for k in range(1, fanout + 1)]
    return {"blob": blob, "fanout": fanout, "type": "BE", "label": "B", "dst": dst}


def main():
    assert os.path.isfile(os.path.join(REF, SRC)), __doc__.split("\n")[2]
    fns = methods()
    cases = []
    graphs = {}
    for method, name, graph, cfg, literals, line in CALLS:
        have = constants(fns[method])
        for lit in literals:
            assert lit in have, f"{method}: {lit!r} not found (cited from line {line})"
        case = {"name": name, "line": f"{SRC}:{line}", "call": cfg}
        if graph[0] == "create":
            nodes, edges = create_graphs(fns[method])[graph[1]]
            case["nodes"], case["edges"] = nodes, edges
        else:
            key = graph[1:]
            if key not in graphs:
                graphs[key] = branchy(fns, *key)
            case["branchy"] = f"{key[0]}x{key[1]}"
        cases.append(case)
    doc = {
        "source": f"{SRC} of the reference: the graphs, calls and asserted results of its tests 08, 09, 10, 11 and 16 that leave "
                  "algo.SPpaths' single-path branch, and test 08's algo.SSpaths call",
        "format": "a case has either nodes: [name, label] in creation order (node id = index) and edges: [src, type, dst, "
                  "attributes] in creation order (relationship id = index), or branchy: a key of `branchy` — blob nodes v = 1 .. "
                  "blob with node id v - 1, then node v = 0 with node id blob, and relationship number i (id i, type `type`) "
                  "from v = 1 + i // fanout to v = dst[i]; source / target of such a case are v values.  call: proc sp = "
                  "algo.SPpaths, ss = algo.SSpaths (target null); types = relTypes ([] = not given), direction = relDirection, "
                  "weight = weightProp, cost = costProp, max_len = maxLen, max_cost = maxCost (null = not given), path_count = "
                  "pathCount.  expect: rows = the asserted row count, weights_desc = the asserted pathWeights in descending "
                  "order within delta, lengths_sorted = the asserted sorted path lengths",
        "branchy": {f"{k[0]}x{k[1]}": v for k, v in graphs.items()},
        "cases": cases,
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, len(cases), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
