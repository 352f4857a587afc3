"""algo.maxFlow's solve through the GraphBLAS + LAGraph C ABI (tests/shim/replay_maxflow_rs.c, written against the transcribed
bindgen declarations only): GrB_Matrix_new(GrB_FP64), GrB_Matrix_build_FP64 with GrB_MAX_FP64, GrB_Matrix_wait, LAGraph_New,
LAGraph_Cached_AT, LAGraph_Cached_EMin, LAGr_MaxFlow(&f, &flow_mtx, NULL, G, src, sink, msg), GrB_Matrix_nvals +
GrB_Matrix_extractTuples_FP64 on the flow, the frees — with one source and sink, with a super source and sink, and over a BOOL
matrix; the printed flow is certified by tests/maxflow_check.py.  Then the refused forms, and nothing of the caller's allocator
left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maxflow_check import certify, dinic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "falkordb_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "replay_maxflow_rs.c")
U64 = np.uint64


def _link(exe):
    from falkordb_amd import build as fb
    fb.build_shim()
    return subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror=implicit-function-declaration",
                           "-I" + os.path.join(ROOT, "tests", "shim"), SRC, "-o", exe, "-L" + LIBDIR,
                           "-llagraphx", "-llagraph", "-lgraphblas", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                          capture_output=True, text=True)


def _defined(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_replay_maxflow_links_against_the_three_libraries(tmp_path):
    r = _link(str(tmp_path / "replay_maxflow_rs"))
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_libraries_define_the_maxflow_names():
    from falkordb_amd import build as fb
    so = fb.build_shim()
    assert "GrB_MAX_FP64" in _defined(so)
    assert "LAGraph_Cached_EMin" in _defined(os.path.join(LIBDIR, "liblagraph.so"))
    assert "LAGr_MaxFlow" in _defined(os.path.join(LIBDIR, "liblagraphx.so"))


def _network(rng):
    """300 inner vertices (ids 2..301) with random integer capacities; 0 = a super source over 8 of them, 1 = a super sink over
    10, arcs of 2^31 - 1 as the procedure adds them.  Some positions are listed twice: GrB_MAX_FP64 keeps the larger."""
    inner, n = 300, 302
    key = np.unique(rng.integers(0, inner * inner, 1800))
    rows, cols = 2 + key // inner, 2 + key % inner
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    caps = rng.integers(1, 200, len(rows)).astype(np.float64) / 4
    big = float(2**31 - 1)
    starts, ends = np.arange(2, 10), np.arange(150, 160)
    rows = np.concatenate([np.zeros(len(starts), dtype=np.int64), rows, ends])
    cols = np.concatenate([starts, cols, np.ones(len(ends), dtype=np.int64)])
    caps = np.concatenate([np.full(len(starts), big), caps, np.full(len(ends), big)])
    return n, rows, cols, caps


def _parse_flow(lines, k):
    head = lines[k].split()
    assert head[0] == "flow" and head[2] == "nvals" and head[4] == "emin"
    nf = int(head[3])
    got = [l.split() for l in lines[k + 1:k + 1 + nf]]
    value = np.array([int(head[1], 16)], dtype=U64).view(np.float64)[0]
    fr = np.array([int(x[0]) for x in got], dtype=np.int64)
    fc = np.array([int(x[1]) for x in got], dtype=np.int64)
    fv = np.array([int(x[2], 16) for x in got], dtype=U64).view(np.float64)
    return float(value), fr, fc, fv, head[5:], k + 1 + nf


@pytest.mark.gpu
def test_maxflow_call_sequence_through_the_lagraph_abi(tmp_path):
    exe = str(tmp_path / "replay_maxflow_rs")
    r = _link(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(41)
    n, rows, cols, caps = _network(rng)
    # every tenth arc once more with a smaller capacity, in front of and behind the real one
    dup = np.arange(0, len(rows), 10)
    frows = np.concatenate([rows[dup[::2]], rows, rows[dup[1::2]]])
    fcols = np.concatenate([cols[dup[::2]], cols, cols[dup[1::2]]])
    fcaps = np.concatenate([caps[dup[::2]] / 2, caps, caps[dup[1::2]] / 4])
    single = (int(rows[20]), int(cols[-30]))
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {len(frows)}\n")
        f.writelines(f"{i} {j} {x:016x}\n" for i, j, x in zip(frows.tolist(), fcols.tolist(), fcaps.view(U64).tolist()))
        f.write(f"flow 0 1\nflow {single[0]} {single[1]}\nboolflow 0 1\nerrors 0 1\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    k = 0
    for (src, sink), ref in (((0, 1), caps), (single, caps), ((0, 1), np.ones(len(caps)))):
        value, fr, fc, fv, emin, k = _parse_flow(lines, k)
        print(f"src={src} sink={sink} value={value!r} flow entries={len(fr)}")
        assert emin == ["1", "0"]                                              # G->emin set, emin_state = LAGraph_VALUE
        certify(n, rows, cols, ref, src, sink, value, fr, fc, fv)
        assert value == dinic(n, rows, cols, ref, src, sink)
    first = dinic(n, rows, cols, caps, 0, 1)
    assert first > 0
    errs = {}
    while lines[k].startswith("errors "):
        parts = lines[k].split()
        errs[parts[1]] = parts[2:]
        k += 1
    assert errs["uncached_at"] == ["-1003", "1", "message"]                    # LAGRAPH_NOT_CACHED; flow_mtx cleared
    assert errs["uncached_emin"] == ["-1003", "1", "message"]
    assert errs["bad_src"] == ["-4", "1"]                                      # GrB_INVALID_INDEX
    assert errs["bad_sink"] == ["-4", "1"]
    assert errs["src_is_sink"] == ["-3", "1"]                                  # GrB_INVALID_VALUE
    assert errs["res_mtx"] == ["-8", "1", "1", "message"]                      # GrB_NOT_IMPLEMENTED, loudly
    assert errs["null_graph"] == ["-2", "1"]                                   # GrB_NULL_POINTER
    assert errs["emin_null_graph"] == ["-2"]
    assert errs["null_flow_mtx"] == ["0", f"{np.array([first]).view(U64)[0]:016x}"]
    assert errs["empty_matrix"] == ["0", "0", "-1", "0", "0"]                  # no entry: emin stays unknown, flow 0 and empty
    assert errs["uint64_matrix"] == ["-8"]
    assert errs["build_dup_max"] == ["0", "5", "2"]
    assert lines[k].split() == ["capacities", str(len(rows))]
    assert lines[k + 1].split() == ["allocator_blocks", "0"]
