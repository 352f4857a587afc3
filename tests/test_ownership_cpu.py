"""CPU: MatRef of falkordb_amd/csrc/common.hpp releases what it holds exactly once, and it is the only place outside mat.hip
that names mat_release: every temporary snapshot of the engine is held by one."""
import os
import subprocess

from falkordb_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falkordb_amd", "csrc")


def test_matref_releases_once_on_every_way_out(tmp_path):
    """tests/host/matref_check.cpp asserts it, with a counting mat_release of its own, under the address and
    undefined-behaviour sanitizers of the HOST side, as a child process (nothing sanitized is loaded into this interpreter).
    The program makes no HIP call: it needs no GPU."""
    exe = str(tmp_path / "matref_check")
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "matref_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"


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
