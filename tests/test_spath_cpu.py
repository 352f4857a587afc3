"""CPU: the checker of shortestPath() (tests/spath_check.py) gives the node lists the reference's flow tests assert
(tests/golden/shortest_path_flow.json) and the two pinned paths of the contract; the new call is declared, exported and bound at
every layer.  No GPU."""
import json
import os
import re
import subprocess

import spath_check
from falkordb_amd import _ffi, build, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "shortest_path_flow.json")))

POSITION = dict(n=13, edges=[(0, 1), (0, 2), (1, 9), (2, 3), (9, 5), (3, 5), (5, 10), (5, 11), (5, 12), (10, 8), (11, 8), (12, 8)],
                query=(0, 8), path=[0, 1, 9, 5, 10, 8])
VERTEX_COUNT = dict(n=6, edges=[(0, 0), (0, 2), (0, 3), (1, 5), (2, 0), (2, 4), (3, 1), (4, 5)], query=(0, 5), path=[0, 2, 4, 5])


def _exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "falkordb_amd", "lib", lib)], capture_output=True,
                         text=True, check=True).stdout
    return set(re.findall(r" T ([a-z0-9_]+)", out))


def test_the_golden_names_what_it_covers():
    assert [c["name"] for c in GOLDEN["cases"]] == ["02_left_to_right", "02_right_to_left", "03_every_source", "04_max_hops_1",
                                                    "05_min_hops_0", "06_both_types", "06_one_type"]
    assert any(s.startswith("test01") for s in GOLDEN["not_covered"]) and any(s.startswith("test07") for s in GOLDEN["not_covered"])


def test_checker_gives_the_goldens_node_lists():
    edges = [(i, t, s, d) for i, (s, t, d) in enumerate(GOLDEN["graph"]["edges"])]
    rows = 0
    for case in GOLDEN["cases"]:
        for src, dst, want in case["rows"]:
            got = spath_check.reference_path(edges, src, dst, case["types"], case["directed"], case["min_hops"], case["max_hops"])
            assert (got[0] if got else None) == want, (case["name"], src, dst)
            if got:
                assert len(got[1]) == len(got[0]) - 1
                for (u, v), e in zip(zip(got[0], got[0][1:]), got[1]):
                    assert edges[e][2:] == (u, v) and (not case["types"] or edges[e][1] in case["types"])
            rows += 1
    assert rows == 2 + 5 + 5 + 5 + 2


def test_parent_is_the_first_frontier_position_not_the_least_id():
    g = POSITION
    path, st = spath_check.shortest_path(g["n"], [s for s, _ in g["edges"]], [d for _, d in g["edges"]], *g["query"])
    assert path == g["path"]
    assert st[5] in path and st[7] == 0 and st[0] + st[1] >= 3


def test_the_side_is_chosen_by_vertex_count_not_entry_count():
    g = VERTEX_COUNT
    path, st = spath_check.shortest_path(g["n"], [s for s, _ in g["edges"]], [d for _, d in g["edges"]], *g["query"])
    assert path == g["path"]


def test_checker_edges_of_the_contract():
    rows, cols = [0, 0, 1, 2], [1, 2, 3, 3]   # the diamond: the meeting vertex is the first key
    path, st = spath_check.shortest_path(4, rows, cols, 0, 3)
    assert path == [0, 1, 3] and st[5] == 1 and st[6] == 2
    assert spath_check.shortest_path(4, rows, cols, 0, 0) == (None, [0, 0, 0, 0, 0, spath_check.NO_MEET, 0, 0])
    assert spath_check.shortest_path(4, rows, cols, 0, 3, 0)[0] is None
    assert spath_check.shortest_path(4, rows, cols, 0, 3, 1)[0] is None
    assert spath_check.shortest_path(4, rows, cols, 0, 3, 2)[0] == [0, 1, 3]
    assert spath_check.shortest_path(4, rows, cols, 3, 0)[0] is None
    assert spath_check.shortest_path(4, rows, cols, 3, 0, -1, True)[0] == [3, 1, 0]
    assert spath_check.shortest_path(4, [], [], 0, 3) == (None, [1, 0, 0, 0, 0, spath_check.NO_MEET, 0, 0])
    # eval_row's edges: Null endpoints, the one-node path, the (v, u) fallback, a type that does not exist
    edges = [(0, "A", 0, 1), (1, "A", 0, 1), (2, "B", 2, 1)]
    assert spath_check.reference_path(edges, None, 1, []) is None
    assert spath_check.reference_path(edges, 1, 1, [], min_hops=0) == ([1], [])
    assert spath_check.reference_path(edges, 1, 1, [], min_hops=1) is None
    assert spath_check.reference_path(edges, 0, 1, []) == ([0, 1], [0])
    assert spath_check.reference_path(edges, 0, 2, [], directed=False) == ([0, 1, 2], [0, 2])
    assert spath_check.reference_path(edges, 0, 1, ["B", "A"]) == ([0, 1], [0])
    assert spath_check.reference_path(edges, 0, 1, ["NONE"]) is None


def test_engine_symbol_is_declared_exported_and_bound():
    build.build_lib()
    with open(os.path.join(ROOT, "include", "fgpu.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bfgpu_shortest_path_batch\s*\(", header)
    assert re.search(r"#define\s+FGPU_SPATH_SLOTS_MAX\s+64\b", header)
    assert "fgpu_shortest_path_batch" in _exported("libfgpu.so")
    assert len(_ffi.SIGNATURES["fgpu_shortest_path_batch"][1]) == 12
    from falkordb_amd import engine
    assert callable(engine.shortest_path_batch)
    assert "spath_batch.hip" in build.SOURCES


def test_host_layer_entries_are_declared_exported_and_reach_the_engine():
    build.build_host()
    for name in ("fh_shortest_path", "fh_shortest_path_batch"):
        assert name in host.declared_symbols(), name
        assert name in _exported("libfalkor_host.so"), name
    assert callable(host.Graph.shortest_path) and callable(host.Graph.shortest_path_batch)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "falkordb_amd", "lib", "libfalkor_host.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "fgpu_shortest_path_batch" in set(re.findall(r" U (fgpu_[a-z0-9_]+)", out))
