"""algo.labelPropagation's call sequence through the GraphBLAS + LAGraph C ABI (tests/shim/replay_cdlp_rs.c, written against
the transcribed bindgen declarations only): GrB_Matrix_dup + GrB_Matrix_resize, LAGraph_New(UNDIRECTED) with
is_symmetric_structure = TRUE, LAGraph_cdlp, GrB_Vector_extractTuples_INT64, the frees — a dense INT64 vector of the labels
of tests/cdlp_check.py, and nothing of the caller's allocator left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cdlp_check import cdlp_labels, csr_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_cdlp_rs.c")


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def test_replay_cdlp_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_cdlp_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.gpu
def test_cdlp_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_cdlp_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(11)
    n = 5000
    m = 9000
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    rows, cols = np.concatenate([a, b, [17]]), np.concatenate([b, a, [17]])     # the symmetric pattern (a self-loop too)
    pairs = sorted(set(zip(rows.tolist(), cols.tolist())))
    resized = n + 40                                                             # node_count + deleted_nodes_count
    runs = [(n, 10), (resized, 10), (n, 1), (resized, 3)]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {len(pairs)}\n")
        f.writelines(f"{i} {j}\n" for i, j in pairs)
        f.writelines(f"cdlp {size} {it}\n" for size, it in runs)
        f.write("errors\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rp, ci = csr_of(n, [p[0] for p in pairs], [p[1] for p in pairs])
    k = 0
    for size, it in runs:
        want, _, _ = cdlp_labels(n, rp, ci, it)
        head = lines[k].split()
        assert head == ["cdlp", str(size), "nvals", str(size)]                 # a dense vector
        got = np.array([[int(x) for x in l.split()] for l in lines[k + 1:k + 1 + size]], dtype=np.int64)
        assert got[:, 0].tolist() == list(range(size))
        full = np.concatenate([want, np.arange(n, size)])                        # the added ids are isolated: they keep their id
        assert np.array_equal(got[:, 1], full)
        k += 1 + size
    errs = {}
    while lines[k].startswith("errors "):
        parts = lines[k].split()
        errs[parts[1]] = parts[2:]
        k += 1
    assert errs["directed"] == ["-8", "1", "message"]                          # GrB_NOT_IMPLEMENTED, loudly
    assert errs["negative_itermax"] == ["-3", "1"]                             # GrB_INVALID_VALUE
    assert errs["null_handle"] == ["-2"] and errs["null_graph"] == ["-2", "1"]  # GrB_NULL_POINTER
    assert errs["zero_itermax"] == ["0", str(n)]
    assert lines[k].split() == ["adjacency", str(len(pairs))]
    assert lines[k + 1].split() == ["allocator_blocks", "0"]
