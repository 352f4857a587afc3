"""CPU: fgpu_node_degrees is declared, exported and bound with one signature; its flags and its window option have the values
include/fgpu.h documents; the host layer declares and exports its two entry points.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_symbol_ctypes_row_and_flags_agree_with_the_header():
    from falkordb_amd import _ffi, build
    hdr = _header("fgpu.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"fgpu_info\s+fgpu_node_degrees\s*\((.*?)\)\s*;", code, flags=re.S)
    assert decl, "include/fgpu.h does not declare fgpu_node_degrees"
    kinds = []
    for p in decl.group(1).split(","):
        p = " ".join(p.split())
        if re.fullmatch(r"fgpu_ctx\* \w+", p):
            kinds.append(_ffi.vp)
        elif re.fullmatch(r"const fgpu_(mat|multi)\* const\* \w+", p):
            kinds.append(_ffi.vpp)
        elif re.fullmatch(r"(const )?uint64_t\* \w+|uint64_t \w+\[8\]", p):
            kinds.append(_ffi.u64p)
        elif re.fullmatch(r"uint64_t \w+", p):
            kinds.append(C.c_uint64)
        elif re.fullmatch(r"int \w+", p):
            kinds.append(C.c_int)
        else:
            raise AssertionError(f"unexpected parameter {p!r}")
    res, args = _ffi.SIGNATURES["fgpu_node_degrees"]
    assert res is C.c_int32 and args == kinds and len(args) == 15
    flags = dict(re.findall(r"#define (FGPU_DEGREE_\w+) (\d+)", hdr))
    assert flags == {"FGPU_DEGREE_OUT": "1", "FGPU_DEGREE_IN": "2"}
    assert (_ffi.FGPU_DEGREE_OUT, _ffi.FGPU_DEGREE_IN) == (1, 2)
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_lib()], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T fgpu_node_degrees$", out, flags=re.M), "libfgpu.so does not export fgpu_node_degrees"
    from falkordb_amd.engine import Context
    assert callable(Context.node_degrees)


def test_window_option_default_and_bounds(tmp_path):
    """degree_window_rows: default 2^24, at least 64, reached by fgpu_set_option / fgpu_get_option under its name — through a
    row of the option table, or through a branch of its own in ctx.hip with the bounds options.hpp names."""
    src = tmp_path / "degree_option.cpp"
    src.write_text('#include <stdio.h>\n#include "options.hpp"\n'
                   'int main() {\n'
                   '    const fgpu::OptRow* r = fgpu::opt_find("degree_window_rows");\n'
                   '    printf("%d %d %lld %lld\\n", fgpu_options().degree_window_rows, r != nullptr, r ? (long long)r->lo : 0ll,\n'
                   '           r ? (long long)r->hi : 0ll);\n'
                   '    return 0;\n}\n')
    exe = str(tmp_path / "degree_option")
    csrc = os.path.join(ROOT, "falkordb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-I", csrc, str(src), "-o", exe], check=True)
    default, in_table, lo, hi = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert default == 1 << 24
    if not in_table:
        with open(os.path.join(csrc, "options.hpp")) as f:
            m = re.search(r"DEGREE_WINDOW_MIN = (\d+), DEGREE_WINDOW_MAX = (?:1 << (\d+)|(\d+));", f.read())
        assert m, "options.hpp names no bounds for degree_window_rows"
        lo, hi = int(m.group(1)), (1 << int(m.group(2))) if m.group(2) else int(m.group(3))
        with open(os.path.join(csrc, "ctx.hip")) as f:
            ctx_src = f.read()
        for fn in ("fgpu_get_option", "fgpu_set_option"):
            body = ctx_src[ctx_src.index("fgpu_info " + fn + "("):]
            body = body[:body.index("\n}\n")]
            assert '"degree_window_rows"' in body, f"{fn} does not know degree_window_rows"
        set_body = ctx_src[ctx_src.index("fgpu_info fgpu_set_option("):]
        assert "DEGREE_WINDOW_MIN" in set_body and "DEGREE_WINDOW_MAX" in set_body
    assert lo == 64 and hi >= 1 << 24
    assert '"degree_window_rows"' in _header("fgpu.h")


def test_host_layer_declares_exports_and_binds_both_entry_points():
    from falkordb_amd import build, host
    hdr = re.sub(r"/\*.*?\*/", "", _header("falkor_host.h"), flags=re.S)
    for name in ("fh_node_degrees", "fh_node_degrees_all"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"include/falkor_host.h does not declare {name}"
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_host()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (fh_[a-z0-9_]+)", out))
    assert {"fh_node_degrees", "fh_node_degrees_all"} <= exported
    assert callable(host.Graph.node_degrees) and callable(host.Graph.node_degrees_all)
