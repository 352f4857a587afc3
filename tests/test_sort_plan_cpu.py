"""CPU: the shape decisions of the stable counting sorts (falkordb_amd/csrc/sort_plan.hpp, plain C++) walked over their whole
domain on the host by tests/host/sort_plan_check.cpp: the digit widths of the staged form, every 32-bit quantity of its
accepted domain, the geometry of the two-level form and its "transpose_wb" override."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_plan_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """built with -fsanitize=address,undefined and run as a child process: nothing sanitized is loaded into this interpreter"""
    exe = str(tmp_path / "sort_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "sort_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, checked = r.stdout.split()
    assert word == "ok" and int(checked) > 20_000


def test_the_plan_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "falkordb_amd", "csrc", "sort_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>", "<stddef.h>"]
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text


def test_transpose_takes_its_shapes_from_the_header():
    """transpose.hip keeps no copy of a decision the check walks"""
    text = open(os.path.join(ROOT, "falkordb_amd", "csrc", "transpose.hip")).read()
    assert '#include "sort_plan.hpp"' in text
    for name in ("constexpr u32 KS_MAX_BUCKETS", "constexpr u32 KP_EB", "constexpr u32 KP_MAX_D", "struct KsGeom", "int kp_widths("):
        assert name not in text, name
    for call in ("kp_widths(", "kp_s_max(", "kp_nb_top(", "kp_nb_max(", "kp_ncnt(", "kp_scatter_lds_bytes(", "kp_accepts("):
        assert call in text, call
