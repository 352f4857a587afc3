"""algo.betweenness' call sequence through the GraphBLAS + LAGraph C ABI (tests/shim/replay_bc_rs.c, written against the
transcribed bindgen declarations only): GrB_Matrix_dup + GrB_Matrix_resize, LAGraph_New(DIRECTED), LAGraph_Cached_AT +
LAGraph_Cached_OutDegree, LAGr_Betweenness, GrB_Vector_extractTuples_FP64, the frees — a dense FP64 vector of the scores the
checker of tests/bc_check.py computes, LAGRAPH_NOT_CACHED without G->AT, GrB_INVALID_INDEX for a source >= n, and nothing of
the caller's allocator left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bc_check import betweenness, csr_of  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_bc_rs.c")


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def test_replay_bc_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_bc_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.gpu
def test_betweenness_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_bc_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(13)
    n = 3000
    m = 9000
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    pairs = sorted(set(zip(rows.tolist(), cols.tolist())) | {(17, 17)})           # a self-loop too
    resized = n + 25                                                               # node_count + deleted_nodes_count
    runs = [(n, list(range(16))), (resized, [5, 9, 5, n + 3, 2999]), (n, [])]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {len(pairs)}\n")
        f.writelines(f"{i} {j}\n" for i, j in pairs)
        for size, src in runs:
            f.write(f"bc {size} {len(src)} {' '.join(map(str, src))}\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rp, ci = csr_of(n, [p[0] for p in pairs], [p[1] for p in pairs])
    k = 0
    for size, src in runs:
        head = lines[k].split()
        assert head == ["bc", str(size), "nvals", str(size)]                    # a dense vector
        got = np.array([[float(x) for x in l.split()] for l in lines[k + 1:k + 1 + size]])
        assert got[:, 0].tolist() == list(range(size))
        rp2 = np.concatenate([rp, np.full(size - n, rp[-1])])                    # the added ids are isolated
        want = betweenness(size, rp2, ci, src)[0]
        assert (np.abs(got[:, 1] - want) <= 1e-9 * np.maximum(1.0, np.abs(want))).all()
        k += 1 + size
    assert lines[k].split() == ["no_at", "-1003"]                                # LAGRAPH_NOT_CACHED
    assert lines[k + 1].split() == ["bad_source", "-4"]                          # GrB_INVALID_INDEX
    assert lines[k + 2].split() == ["adjacency", str(len(pairs))]
    assert lines[k + 3].split() == ["allocator_blocks", "0"]
