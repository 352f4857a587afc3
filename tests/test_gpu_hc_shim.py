"""algo.HarmonicCentrality's call sequence through the GraphBLAS + LAGraph C ABI (tests/shim/replay_hc_rs.c, written against the
transcribed bindgen declarations only): GrB_Matrix_new + GrB_Matrix_eWiseMult_BinaryOp(GrB_ONEB_BOOL) + GrB_Matrix_resize,
LAGraph_New(DIRECTED), GrB_Vector_new + GrB_Vector_assign_BOOL(GrB_ALL), LAGr_HarmonicCentrality,
GrB_Vector_extractTuples_FP64 / _INT64, the frees — full FP64 / INT64 vectors holding the scores and reachable counts of
tests/hc_check.py (scores within 1e-9, reachable equal), and nothing of the caller's allocator left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hc_check import csr_of, harmonic, round_margin  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_hc_rs.c")


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def test_replay_hc_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_hc_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


def test_libgraphblas_defines_the_names_the_procedure_adds():
    from falkordb_amd import build as fb
    so = fb.build_shim()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("GrB_ONEB_BOOL", "GrB_Matrix_eWiseMult_BinaryOp", "GrB_Vector_assign_BOOL", "GrB_ALL"):
        assert name in have, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "liblagraphx.so")], capture_output=True, text=True,
                         check=True).stdout
    assert "LAGr_HarmonicCentrality" in {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.mark.gpu
def test_hc_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_hc_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(11)
    n = 2000
    m = 5000
    rows, cols = np.append(rng.integers(0, n, m), 17), np.append(rng.integers(0, n, m), 17)   # directed; a self-loop too
    pairs = sorted(set(zip(rows.tolist(), cols.tolist())))
    resized = n + 40                                                             # node_count + deleted_nodes_count
    runs = [n, resized]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {len(pairs)}\n")
        f.writelines(f"{i} {j}\n" for i, j in pairs)
        f.writelines(f"hc {size}\n" for size in runs)
        f.write("errors\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    k = 0
    for size in runs:
        # the added ids are isolated vertices; their hashes are those of their own indices
        rp, ci = csr_of(size, [p[0] for p in pairs], [p[1] for p in pairs])
        assert round_margin(size, rp, ci) > 1e-6
        ws, wr, _, _ = harmonic(size, rp, ci)
        assert lines[k].split() == ["hc", str(size), "nvals", str(size), str(size)]   # two full vectors
        rowsets = [l.split() for l in lines[k + 1:k + 1 + size]]
        assert [int(x[0]) for x in rowsets] == list(range(size))
        score = np.array([float(x[1]) for x in rowsets])
        reach = np.array([int(x[2]) for x in rowsets], dtype=np.int64)
        err = float(np.abs(score - ws).max())
        print("hc", size, "largest score difference", err)
        assert err <= 1e-9
        assert np.array_equal(reach, wr)
        assert (score[n:] == 0.0).all() and (reach[n:] == 0).all()
        k += 1 + size
    errs = {}
    while lines[k].startswith("errors "):
        parts = lines[k].split()
        errs[parts[1]] = parts[2:]
        k += 1
    assert errs["null_scores"] == ["-2", "1"]                                  # GrB_NULL_POINTER; reachable_nodes cleared
    assert errs["false_weight"] == ["-8", "1", "1", "message"]                 # GrB_NOT_IMPLEMENTED, loudly
    assert errs["sparse_weights"] == ["-8", "1", "1", "message"]
    assert errs["long_weights"] == ["-8", "1", "1", "message"]
    assert errs["null_graph"] == ["-2", "1", "1"]
    assert errs["null_reachable"] == ["0", str(n)]
    assert errs["null_weights"] == ["0", str(n)]
    assert errs["set_weights"] == ["0", str(n)]
    assert errs["ewise_other_op"] == ["-8"] and errs["assign_index_list"] == ["-8"]
    assert lines[k].split() == ["adjacency", str(len(pairs))]
    assert lines[k + 1].split() == ["allocator_blocks", "0"]
