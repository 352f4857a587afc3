#!/usr/bin/env python3
"""Generate tests/golden/shortest_path_flow.json from the reference's tests/flow/test_shortest_path.py.

usage: make_shortest_path_golden.py <root of the reference tree>
Runs ONLY where the reference tree is present (like make_asp_golden.py); the emitted JSON is committed, so pytest never reads
the reference.  Covered: the calls of that file that evaluate shortestPath() between bound nodes:
  test02  both directions                     test03  every source to one destination
  test04  *..1                                test05  *0..
  test06  :E|:E2 and :E
Not covered: test01 (parser errors; its one evaluated query, an unknown type, is covered by the host tests) and test07 (where
in a query the pattern may stand).
What is read from the reference at run time: the CREATE statement of populate_graph (node id = the order the nodes are
created in, relationship id = the order of the relationships), and from each covered test method the query strings and the
literals assigned to `expected_result`, evaluated with `nodes[i]` = node id i.  A method that runs more queries than it states
expectations for (test02 compares its second query with the first one's) reuses the last one.  The CASES below name every
query by method and position, with the pattern text it is expected to hold."""
import ast
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FALKORDB_REFERENCE", "")
SRC = "tests/flow/test_shortest_path.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shortest_path_flow.json")

# (method, position among the method's queries, case name, cited pattern literal)
CASES = [
    ("test02_simple_shortest_path", 0, "02_left_to_right", "shortestPath((a)-[*]->(d))"),
    ("test02_simple_shortest_path", 1, "02_right_to_left", "shortestPath((b)<-[*]-(a))"),
    ("test03_shortest_path_multiple_results", 0, "03_every_source", "shortestPath((a)-[*]->(b))"),
    ("test04_max_hops", 0, "04_max_hops_1", "shortestPath((a)-[*..1]->(b))"),
    ("test05_min_hops", 0, "05_min_hops_0", "shortestPath((a)-[*0..]->(b))"),
    ("test06_restricted_reltypes", 0, "06_both_types", "shortestPath((a)-[:E|:E2*]->(b))"),
    ("test06_restricted_reltypes", 1, "06_one_type", "shortestPath((a)-[:E*]->(b))"),
]
NOT_COVERED = ["test01_invalid_shortest_paths: parser errors",
               "test07_shortestPath_in_filter: pattern placement and unbound endpoints"]


def methods():
    tree = ast.parse(open(os.path.join(REF, SRC)).read())
    return {f.name: f for cls in tree.body if isinstance(cls, ast.ClassDef) for f in cls.body if isinstance(f, ast.FunctionDef)}


def assigned(fn, name):
    """the values assigned to `name` in fn, in source order, as AST nodes"""
    out = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id == name:
            out.append(node)
    return [n.value for n in sorted(out, key=lambda n: n.lineno)]


def graph_of(fn):
    q = ast.literal_eval(assigned(fn, "q")[0])
    alias, vs = {}, []
    for a, v in re.findall(r"CREATE \((\w+):L \{v:(\d+)\}\)", q):
        alias[a] = len(vs)
        vs.append(int(v))
    edges = [[alias[a], t, alias[b]] for a, t, b in re.findall(r"CREATE \((\w+)\)-\[:(\w+)\]->\((\w+)\)", q)]
    return {"nodes": [{"v": v} for v in vs], "edges": edges}


def main():
    assert os.path.isfile(os.path.join(REF, SRC)), __doc__.split("\n")[2]
    fns = methods()
    graph = graph_of(fns["populate_graph"])
    by_v = {n["v"]: i for i, n in enumerate(graph["nodes"])}
    everyone = list(range(len(graph["nodes"])))
    cases = []
    for method, pos, name, literal in CASES:
        fn = fns[method]
        queries = [ast.literal_eval(v) for v in assigned(fn, "query")]
        expects = [eval(compile(ast.Expression(v), SRC, "eval"), {"nodes": everyone}) for v in assigned(fn, "expected_result")]
        query, expected = queries[pos], expects[min(pos, len(expects) - 1)]
        assert literal in query, f"{method}: {literal!r} not found in its query {pos}"
        left, larrow, rel, rarrow, right = re.search(r"shortestPath\(\((\w+)\)(<?)-\[([^\]]*)\]-(>?)\((\w+)\)\)", query).groups()
        assert bool(larrow) != bool(rarrow), name
        types = re.findall(r":(\w+)", rel)
        hops = re.search(r"\*(\d*)(\.\.)?(\d*)", rel).groups()
        min_hops = int(hops[0]) if hops[0] else 1
        max_hops = int(hops[2]) if hops[2] else (min_hops if hops[0] and not hops[1] else None)
        s_var, d_var = (right, left) if larrow else (left, right)   # the arrow's source is the search's source

        def bound(var):
            m = re.search(r"\(" + var + r" \{v: (\d+)\}\)", query)
            return [by_v[int(m.group(1))]] if m else everyone   # MATCH (a): every node, ORDER BY a
        srcs, dsts = bound(s_var), bound(d_var)
        assert len(dsts) == 1, name
        if len(srcs) == 1:      # UNWIND nodes(p) AS n RETURN n.v: one row per node of the one path
            rows = [[srcs[0], dsts[0], [by_v[r[0]] for r in expected]]]
        else:                   # RETURN a, nodes(p) ORDER BY a
            assert [r[0] for r in expected] == srcs, name
            rows = [[r[0], dsts[0], r[1]] for r in expected]
        cases.append({"name": name, "line": f"{SRC}:{fn.lineno}-{fn.end_lineno}", "pattern": literal, "types": types,
                      "directed": True, "min_hops": min_hops, "max_hops": max_hops, "rows": rows})
    doc = {
        "source": f"{SRC} of the reference: the graph its populate method builds, the shortestPath() calls of its tests 02 to 06 "
                  "and the results they assert",
        "format": "graph: nodes in creation order (node id = index), edges [src, type, dst] in creation order (relationship id = "
                  "index); a case: the pattern's types in order ([] = none named), min_hops 0 or 1, max_hops null = unbounded, "
                  "rows = [src, dst, the asserted nodes(p) as node ids or null] with src the arrow's source",
        "not_covered": NOT_COVERED,
        "graph": graph,
        "cases": cases,
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(OUT, len(cases), "cases")


if __name__ == "__main__":
    main()
