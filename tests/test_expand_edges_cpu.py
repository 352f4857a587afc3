"""CPU: the relationship-emitting CondTraverse batch is declared, exported and bound at every layer, its handle has one owner,
and that owner frees once in the shapes the host layer holds it.  No GPU."""
import os
import re
import subprocess

from falkordb_amd import _ffi, build, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("fgpu_multi_new", "fgpu_multi_free", "fgpu_multi_size", "fgpu_expand_edges")


def _exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "falkordb_amd", "lib", lib)], capture_output=True,
                         text=True, check=True).stdout
    return set(re.findall(r" T ([a-z0-9_]+)", out))


def test_engine_symbols_are_declared_exported_and_bound():
    build.build_lib()
    with open(os.path.join(ROOT, "include", "fgpu.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exported = _exported("libfgpu.so")
    for name in ENGINE:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in fgpu.h"
        assert name in exported, name + " is not exported by libfgpu.so"
        assert name in _ffi.SIGNATURES, name + " has no ctypes signature"
    assert len(_ffi.SIGNATURES["fgpu_expand_edges"][1]) == 22
    for flag, value in (("FGPU_EDGES_TRANSPOSED", 1), ("FGPU_EDGES_BIDIRECTIONAL", 2), ("FGPU_EDGES_FIRST_ONLY", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), header), flag
    from falkordb_amd import engine
    assert callable(engine.Context.multi_new) and callable(engine.Context.expand_edges)


def test_host_layer_entry_is_declared_exported_and_reaches_the_engine():
    build.build_host()
    assert "fh_cond_traverse_edges_batch" in host.declared_symbols()
    assert "fh_cond_traverse_edges_batch" in _exported("libfalkor_host.so")
    assert callable(host.Graph.cond_traverse_edges_batch)
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "falkordb_amd", "lib", "libfalkor_host.so")],
                         capture_output=True, text=True, check=True).stdout
    used = set(re.findall(r" U (fgpu_[a-z0-9_]+)", out))
    assert {"fgpu_expand_edges", "fgpu_multi_new", "fgpu_multi_free"} <= used


def test_the_new_entry_declines_what_stays_per_row_without_a_device():
    """the eligibility rule of the reference stands beside the new one (no graph, no GPU: the spec alone decides it)"""
    L = host.load()
    for kw in (dict(emit=True), dict(bidir=True), dict(siblings=True)):
        assert L.fh_cond_traverse_eligible(host.cond_spec(hops=[(["R"], [])], **kw)) == 0


def test_only_owned_hpp_frees_a_multi_edge_table():
    naming = []
    for d in ("host", "shim"):
        for f in sorted(os.listdir(os.path.join(ROOT, "falkordb_amd", d))):
            if "fgpu_multi_free" in open(os.path.join(ROOT, "falkordb_amd", d, f)).read():
                naming.append(f)
    assert naming == ["owned.hpp"], naming


def test_multiref_frees_once_alone_and_shared_by_tensor_copies(tmp_path):
    """tests/host/multiref_check.cpp, built with the host sanitizers and run as a stand-alone program"""
    exe = str(tmp_path / "multiref_check")
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "multiref_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
