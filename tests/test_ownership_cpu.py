"""CPU: MatRef of falkordb_amd/csrc/common.hpp releases what it holds exactly once, and it is the only place outside mat.hip
that names mat_release: every temporary snapshot of the engine is held by one.  DevBuf does the same for device memory:
every cached index of a snapshot is one, and no file below the matrix layer allocates or frees a block by hand.  The host layer
above the C ABI does the same with SnapshotRef, PlanRef and EngineBuf of falkordb_amd/host/owned.hpp."""
import os
import subprocess

from falkordb_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falkordb_amd", "csrc")


def _run_host_check(tmp_path, name):
    """tests/host/<name>.cpp built with the address and undefined-behaviour sanitizers of the HOST side and run as a child
    process (nothing sanitized is loaded into this interpreter).  The program makes no HIP call: it needs no GPU."""
    exe = str(tmp_path / name)
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"


def test_matref_releases_once_on_every_way_out(tmp_path):
    """tests/host/matref_check.cpp asserts it, with a counting mat_release of its own."""
    _run_host_check(tmp_path, "matref_check")


def test_devbuf_frees_once_alone_and_as_a_member(tmp_path):
    """tests/host/devbuf_check.cpp asserts it, with a counting fgpu_ctx::dev_alloc / dev_free of its own: destruction, take(),
    a second alloc, both moves, a self-move, and fgpu_tiles — whole, half built, and one layout moved over another."""
    _run_host_check(tmp_path, "devbuf_check")


def test_host_owners_free_once_on_every_way_out(tmp_path):
    """tests/host/owned_check.cpp asserts it for SnapshotRef, PlanRef and EngineBuf<T> (the seven element types in use), with
    counting engine functions of its own: destruction, out(), release(), reset(), both moves, a self-move, a growing vector,
    a failed alloc(), the context fgpu_free receives, and an exception between out() and the end of the scope."""
    _run_host_check(tmp_path, "owned_check")


def test_only_the_holder_and_mat_hip_name_mat_release():
    """A function that builds a snapshot holds it in a MatRef from mat_alloc until `*out = ref.release()`, so no file but
    common.hpp (the holder) and mat.hip (the definition, the public free, the transpose cache) releases one by hand."""
    naming, rel = [], []
    for f in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, f)).read()
        if "mat_release(" in src:
            naming.append(f)
        if "struct Rel" in src:
            rel.append(f)
    assert naming == ["common.hpp", "mat.hip"], naming
    assert "spgemm.hip" not in rel, rel


def test_only_the_holder_the_pool_and_mat_hip_name_dev_alloc():
    """Device memory below fgpu_mat is held by a DevBuf from its allocation on: only common.hpp (the holder), ctx.hip (the pool)
    and mat.hip (the four stored arrays of a snapshot) name dev_alloc / dev_free, and the hand-kept free lists are gone."""
    raw, text = [], ""
    for f in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, f)).read()
        text += src
        if "dev_alloc(" in src or "dev_free(" in src:
            raw.append(f)
    assert raw == ["common.hpp", "ctx.hip", "mat.hip"], raw
    for gone in ("xp_free_buffers", "blocked_release", "pr_parts_release(", "bc_cached_transpose"):
        assert gone not in text, gone


def test_only_owned_hpp_frees_or_pins_in_the_host_layer():
    """Above the C ABI every engine handle is held by an owner of owned.hpp from the call that makes it: no other file of
    falkordb_amd/host or falkordb_amd/shim names fgpu_mat_free or fgpu_bfs_plan_free at all, or calls fgpu_host_alloc;
    fgpu_free is called by owned.hpp and by graphblas_shim.cpp alone (a GrB_Vector over a pinned block is that block's owner)."""
    names = ("fgpu_mat_free", "fgpu_bfs_plan_free", "fgpu_free(", "fgpu_host_alloc(", "struct EngineArray")
    naming = {n: [] for n in names}
    for d in ("host", "shim"):
        for f in sorted(os.listdir(os.path.join(ROOT, "falkordb_amd", d))):
            src = open(os.path.join(ROOT, "falkordb_amd", d, f)).read()
            for n in names:
                if n in src:
                    naming[n].append(f)
    assert naming["fgpu_mat_free"] == ["owned.hpp"], naming
    assert naming["fgpu_bfs_plan_free"] == ["owned.hpp"], naming
    assert naming["fgpu_free("] == ["owned.hpp", "graphblas_shim.cpp"], naming
    assert naming["fgpu_host_alloc("] == ["owned.hpp"], naming
    assert naming["struct EngineArray"] == [], naming
