"""algo.MSF's forest through the GraphBLAS + LAGraph C ABI (tests/shim/replay_msf_rs.c, written against the transcribed bindgen
declarations only): GrB_Matrix_new(GrB_FP64), GrB_Matrix_build_FP64, GrB_Matrix_wait, LAGraph_msf(.., false, msg),
GrB_Matrix_nvals + GrB_Matrix_extractTuples_FP64 on the forest, GrB_Vector_extractTuples_INT64 on componentId, the frees — the
forest (every edge once at (min, max), weight bits included) and the components of tests/msf_check.py, again after
GrB_Matrix_resize, the refused forms, and nothing of the caller's allocator left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of, msf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_msf_rs.c")
NEW_NAMES = ("GrB_Matrix_build_FP64", "GrB_Matrix_setElement_FP64", "GrB_Matrix_extractElement_FP64",
             "GrB_Matrix_extractTuples_FP64", "GrB_MIN_FP64")


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def test_replay_msf_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_msf_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


def test_libgraphblas_defines_the_fp64_matrix_names():
    from falkordb_amd import build as fb
    so = fb.build_shim()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_NAMES:
        assert name in have, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "liblagraphx.so")], capture_output=True, text=True,
                         check=True).stdout
    assert "LAGraph_msf" in {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.mark.gpu
def test_msf_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_msf_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(31)
    n, m = 2000, 6000
    a, b = rng.integers(0, n, 2 * m), rng.integers(0, n, 2 * m)
    keep = a != b
    key = rng.permutation(np.unique(np.minimum(a, b)[keep] * n + np.maximum(a, b)[keep]))[:m]
    lo, hi = key // n, key % n
    assert len(lo) == m
    w = rng.integers(-6, 6, m).astype(np.float64) * 0.5                     # many ties, both signs, -0.0 among them
    w[rng.random(m) < 0.05] = -0.0
    w[rng.random(m) < 0.02] = np.inf
    bits = bits_of(w)
    resized = n + 40
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {m}\n")
        f.writelines(f"{i} {j} {x:016x}\n" for i, j, x in zip(lo.tolist(), hi.tolist(), bits.tolist()))
        f.write(f"msf\nresize {resized}\nmsf\nerrors\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    rows, cols, both = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([bits, bits])
    k = 0
    for size in (n, resized):
        fr, fc, fb, comp = msf(size, rows, cols, both)
        assert lines[k].split() == ["msf", str(size), "nvals", str(len(fr)), str(size)]   # a full component vector
        got = [l.split() for l in lines[k + 1:k + 1 + len(fr)]]
        assert [int(x[0]) for x in got] == fr.tolist() and [int(x[1]) for x in got] == fc.tolist()
        assert [int(x[2], 16) for x in got] == fb.tolist()
        k += 1 + len(fr)
        got = [l.split() for l in lines[k:k + size]]
        assert [int(x[0]) for x in got] == list(range(size))
        assert [int(x[1]) for x in got] == comp.tolist()
        k += size
    nforest = len(msf(resized, rows, cols, both)[0])
    errs = {}
    while lines[k].startswith("errors "):
        parts = lines[k].split()
        errs[parts[1]] = parts[2:]
        k += 1
    assert errs["null_forest"] == ["-2", "1"]                                  # GrB_NULL_POINTER; componentId cleared
    assert errs["null_a"] == ["-2", "1", "1"]
    assert errs["sanitize"] == ["-8", "1", "1", "message"]                     # GrB_NOT_IMPLEMENTED, loudly
    assert errs["uint64_matrix"] == ["-8", "1", "1", "message"]
    assert errs["non_square"] == ["-6", "1", "1"]                              # GrB_DIMENSION_MISMATCH
    assert errs["null_component"] == ["0", str(nforest)]
    assert errs["bool_matrix"] == ["0", "2", "1"]
    assert errs["build_dup_null"] == ["-3"]                                    # GrB_INVALID_VALUE
    assert errs["build_dup_min"] == ["0", "-2.5", "8000000000000000", "1", "2"]   # -0.0 kept bit-exact; (3, 3): GrB_NO_VALUE
    assert errs["tuples_no_room"] == ["-103"]                                  # GrB_INSUFFICIENT_SPACE
    assert lines[k].split() == ["adjacency", str(2 * m)]
    assert lines[k + 1].split() == ["allocator_blocks", "0"]
