"""algo.WCC's call sequence through the GraphBLAS + LAGraph C ABI (tests/shim/replay_wcc_rs.c, written against the
transcribed bindgen declarations only): GrB_Matrix_dup + GrB_Matrix_resize, LAGraph_New(UNDIRECTED) with
is_symmetric_structure = TRUE, LAGr_ConnectedComponents, GrB_Vector_extractTuples_INT64, the frees — a dense INT64 vector of
the smallest vertex id of every component, and nothing of the caller's allocator left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wcc_check import csr_of, wcc_labels  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_wcc_rs.c")


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def test_replay_wcc_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_wcc_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.gpu
def test_wcc_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_wcc_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(11)
    n = 5000
    m = 3000
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    rows, cols = np.concatenate([a, b, [17]]), np.concatenate([b, a, [17]])     # the symmetric pattern (a self-loop too)
    pairs = sorted(set(zip(rows.tolist(), cols.tolist())))
    resized = n + 40                                                             # node_count + deleted_nodes_count
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {len(pairs)}\n")
        f.writelines(f"{i} {j}\n" for i, j in pairs)
        f.write(f"wcc {n}\nwcc {resized}\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rp, ci = csr_of(n, [p[0] for p in pairs], [p[1] for p in pairs])
    want = wcc_labels(n, rp, ci)
    k = 0
    for size in (n, resized):
        head = lines[k].split()
        assert head == ["wcc", str(size), "nvals", str(size)]                  # a dense vector
        got = np.array([[int(x) for x in l.split()] for l in lines[k + 1:k + 1 + size]], dtype=np.int64)
        assert got[:, 0].tolist() == list(range(size))
        full = np.concatenate([want, np.arange(n, size)])                        # the added ids are isolated
        assert np.array_equal(got[:, 1], full)
        k += 1 + size
    assert lines[k].split() == ["adjacency", str(len(pairs))]
    assert lines[k + 1].split() == ["allocator_blocks", "0"]
