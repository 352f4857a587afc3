#!/usr/bin/env python3
"""Generate tests/golden/asp_flow.json from the reference's tests/flow/test_all_shortest_paths.py.

usage: make_asp_golden.py <root of the reference tree>
Runs ONLY where the reference tree is present (like make_sppaths_golden.py); the emitted JSON is committed, so pytest never
reads the reference.  Covered: the calls of that file that reach AllShortestPathsOp in the shape the host operator serves
(both endpoints bound, one variable-length pattern, no attribute filter):
  test02  all three queries (left to right, right to left, undirected)      test05  both directions (no row)
  test06  the cycle, both directions                                        test07  unreachable endpoints, undirected
Not covered: test01 (parser and planner errors), test03 (a fixed hop in front of the variable-length one), test04 (an edge
attribute filter).
What is read from the reference at run time: the two populate methods and the four test methods are compiled out of the file
and run against a stand-in for `self`: Node and Edge stand-ins record what the populate methods create and in which order the
CREATE statement lists it (node id / relationship id = that order), graph.query() records the query text, and env.assertEqual()
records what each query's result is compared with.  The CASES below name every recorded call by method and position, with the
pattern text it is expected to hold: each cited literal is checked to occur in the query recorded from that method.
The asserted node lists are stored as the SETS of relationship ids they traverse: each consecutive node pair of an asserted
list is joined by exactly one relationship of these graphs, in either direction (asserted here), which sidesteps how nodes(p)
orders a reversed cycle."""
import ast
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FALKORDB_REFERENCE", "")
SRC = "tests/flow/test_all_shortest_paths.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "asp_flow.json")

# (method, position among the method's recorded queries, case name, cited pattern literal)
CASES = [
    ("test02_all_shortest_paths", 0, "02_left_to_right", "allShortestPaths((v1)-[*]->(v4))"),
    ("test02_all_shortest_paths", 1, "02_right_to_left", "allShortestPaths((v4)<-[*]-(v1))"),
    ("test02_all_shortest_paths", 2, "02_undirected", "allShortestPaths((v1)-[*]-(v4))"),
    ("test05_all_shortest_no_results", 0, "05_left_to_right", "allShortestPaths((v5)-[*]->(v3))"),
    ("test05_all_shortest_no_results", 1, "05_right_to_left", "allShortestPaths((v3)<-[*]-(v5))"),
    ("test06_all_shortest_cycle", 0, "06_cycle_left_to_right", "allShortestPaths((v1)-[*]->(v1))"),
    ("test06_all_shortest_cycle", 1, "06_cycle_right_to_left", "allShortestPaths((v1)<-[*]-(v1))"),
    ("test07_all_shortest_paths_unreachables", 1, "07_unreachable_undirected", "allshortestpaths((a)-[*]-(k))"),
]
NOT_COVERED = ["test01_invalid_shortest_paths: parser and planner errors, no operator call",
               "test03_all_shortest_multiple_traversals: a fixed hop in front of the variable-length pattern",
               "test04_all_shortest_edge_filter: an edge attribute filter"]


class Node:
    def __init__(self, alias=None, labels=None, properties=None):
        self.alias, self.label, self.props = alias, labels, properties or {}

    def __str__(self):
        return f"<node {id(self)}>"


class Edge:
    def __init__(self, src, relation, dst, properties=None):
        self.src, self.type, self.dst = src, relation, dst

    def __str__(self):
        return f"<edge {id(self)}>"


class GraphRec:
    """stands in for a falkordb Graph: keeps the nodes and edges in the order the CREATE statements list them"""

    def __init__(self, made):
        self.made, self.nodes, self.edges, self.queries = made, [], [], []

    def query(self, q):
        self.queries.append(q)
        if "CREATE" in q:
            for kind, key in re.findall(r"<(node|edge) (\d+)>", q):
                obj = self.made[int(key)]
                (self.nodes if kind == "node" else self.edges).append(obj)
            # anonymous patterns (test07): (:A)-[:R]->(:Z)
            for a, t, b in re.findall(r"\(:(\w+)\)-\[:(\w+)\]->\(:(\w+)\)", q):
                na, nb = Node(labels=a), Node(labels=b)
                self.nodes += [na, nb]
                self.edges.append(Edge(na, t, nb))
        return type("Result", (), {"result_set": []})()


class EnvRec:
    def __init__(self):
        self.asserted = []

    def assertEqual(self, actual, expected):
        self.asserted.append(expected)


class SelfRec:
    pass


def methods():
    tree = ast.parse(open(os.path.join(REF, SRC)).read())
    return {f.name: f for cls in tree.body if isinstance(cls, ast.ClassDef) for f in cls.body if isinstance(f, ast.FunctionDef)}


def compiled(fn, made):
    def node(**kw):
        n = Node(**kw)
        made[id(n)] = n
        return n

    def edge(*a, **kw):
        e = Edge(*a, **kw)
        made[id(e)] = e
        return e
    ns = {"Node": node, "Edge": edge}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), SRC, "exec"), ns)
    return ns[fn.name]


def graph_json(g):
    idx = {id(n): i for i, n in enumerate(g.nodes)}
    return {"nodes": [{"alias": n.alias, "label": n.label, "v": n.props.get("v")} for n in g.nodes],
            "edges": [[idx[id(e.src)], e.type, idx[id(e.dst)]] for e in g.edges]}


def bind(g, query, var):
    """the node a query binds `var` to: (var {v: k}) by property, (var:Label) by label"""
    m = re.search(r"\(" + var + r" \{v: (\d+)\}\)", query)
    if m:
        hits = [i for i, n in enumerate(g.nodes) if n.props.get("v") == int(m.group(1))]
    else:
        m = re.search(r"\(" + var + r":(\w+)\)", query)
        hits = [i for i, n in enumerate(g.nodes) if n.label == m.group(1)]
    assert len(hits) == 1, (var, query)
    return hits[0]


def main():
    assert os.path.isfile(os.path.join(REF, SRC)), __doc__.split("\n")[2]
    fns = methods()
    made = {}
    me = SelfRec()
    me.graph, me.cyclic_graph, me.env = GraphRec(made), GraphRec(made), EnvRec()
    compiled(fns["populate_graph"], made)(me)
    compiled(fns["populate_cyclic_graph"], made)(me)
    graphs = {"acyclic": graph_json(me.graph), "cyclic": graph_json(me.cyclic_graph)}
    cases = []
    for method in dict.fromkeys(m for m, *_ in CASES):
        target = me.cyclic_graph if "cycle" in method else me.graph
        q0, a0 = len(target.queries), len(me.env.asserted)
        compiled(fns[method], made)(me)
        queries, asserted = target.queries[q0:], me.env.asserted[a0:]
        if method.startswith("test07"):
            graphs["acyclic_07"] = graph_json(me.graph)   # the first graph with test07's four nodes added
        for m, pos, name, literal in CASES:
            if m != method:
                continue
            query = queries[pos]
            assert literal in query, f"{method}: {literal!r} not found in its query {pos}"
            expected = asserted[[q for q in queries if "allshortestpaths" in q.lower()].index(query)]
            pat = re.search(r"\((\w+)\)(<?)-\[\*\]-(>?)\((\w+)\)", query)
            left, larrow, rarrow, right = pat.groups()
            rev = larrow == "<"
            gname = "cyclic" if target is me.cyclic_graph else ("acyclic_07" if method.startswith("test07") else "acyclic")
            src, dst = bind(target, query, right if rev else left), bind(target, query, left if rev else right)
            idx = {id(n): i for i, n in enumerate(target.nodes)}
            rows = [] if expected in (0, []) else [[idx[id(n)] for n in row[0]] for row in expected]
            id_sets = []
            for row in rows:
                ids = set()
                for a, b in zip(row, row[1:]):
                    join = [k for k, e in enumerate(target.edges) if {idx[id(e.src)], idx[id(e.dst)]} == {a, b}]
                    assert len(join) == 1, f"{name}: {a} and {b} are joined by {len(join)} relationships"
                    ids.add(join[0])
                assert len(ids) == len(row) - 1, name
                id_sets.append(sorted(ids))
            cases.append({"name": name, "line": f"{SRC}:{fns[method].lineno}-{fns[method].end_lineno}", "graph": gname,
                          "pattern": literal, "src": src, "dst": dst, "types": [], "bidirectional": not (larrow or rarrow),
                          "reversed": rev, "max_hops": None, "expect_nodes": rows, "expect_id_sets": sorted(id_sets)})
    doc = {
        "source": f"{SRC} of the reference: the two graphs its populate methods build, the calls of its tests 02, 05, 06 and "
                  "07 and the results they assert",
        "format": "graphs: nodes in creation order (node id = index), edges [src, type, dst] in creation order (relationship "
                  "id = index); a case: src / dst = the operator's from / to node (the arrow's source and target), reversed = "
                  "the pattern is written right to left, max_hops null = unbounded, expect_nodes = the asserted nodes(p) lists, "
                  "expect_id_sets = the sorted list of the sorted relationship-id sets those lists traverse",
        "not_covered": NOT_COVERED,
        "graphs": graphs,
        "cases": cases,
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(OUT, len(cases), "cases")


if __name__ == "__main__":
    main()
