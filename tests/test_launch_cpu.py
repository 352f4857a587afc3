"""CPU: pick<...>() / pick(bool) of falkordb_amd/csrc/common.hpp name the constant their run-time value stands for, call their
callable once and return what it returns; and every kernel of falkordb_amd/csrc/ is launched through the one launch helper."""
import os
import re
import subprocess

from falkordb_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falkordb_amd", "csrc")


def test_pick_names_the_constant_calls_once_and_returns_the_callables_result(tmp_path):
    """tests/host/pick_check.cpp asserts it under the address and undefined-behaviour sanitizers of the HOST side, as a child
    process (nothing sanitized is loaded into this interpreter).  The program makes no HIP call: it needs no GPU."""
    exe = str(tmp_path / "pick_check")
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "pick_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"


def test_one_launch_site_and_one_attribute_call_in_the_engine():
    launches, raises = [], []
    for f in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, f)).read()
        launches += [f] * len(re.findall(r"\bhipLaunchKernelGGL\b|<<<", src))
        raises += [f] * len(re.findall(r"\bhipFuncSetAttribute\b", src))
    assert launches == ["common.hpp"], launches
    assert raises == ["common.hpp"], raises
