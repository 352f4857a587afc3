"""CPU: the option table of falkordb_amd/csrc/options.hpp keeps every name, bound and default the engine had before the table
existed, include/fgpu.h documents exactly those names, and engine.Context refuses a malformed FGPU_OPTS before it opens anything."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, kind, lo, hi, default) of every settable option.  Written down from the strcmp ladder of fgpu_set_option and the struct
# defaults as they stood before the table (one deliberate change: expand_scan_min stops at 2^31 - 1, the ladder let 2^31 into an
# int), NOT from the table: a new option adds a line here.  bool = any value, stored as value != 0.
OPTIONS = [
    ("tiled_u", "pow2", 1, 8, 8),
    ("tiled_nt", "bool", 0, 1, 0),
    ("tiled_threads", "pow2", 256, 1024, 1024),
    ("tiled_wgs", "range", 0, 65536, 0),
    ("expand_mode", "range", 0, 2, 0),
    ("expand_row_groups", "bool", 0, 1, 1),
    ("expand_fuse_count", "bool", 0, 1, 1),
    ("expand_bits_ratio", "range", 1, 1024, 28),
    ("blocked_variant", "range", 0, 3, 0),
    ("tiled_layout", "range", 0, 2, 0),
    ("bfs_wgs_per_cu", "range", 1, 64, 6),
    ("bfs_tiny", "range", 0, 2, 2),
    ("bfs_hub_first", "bool", 0, 1, 1),
    ("bfs_alive_rule", "bool", 0, 1, 1),
    ("bfs_pb", "range", 0, 2, 1),
    ("bfs_pb_min_edges", "range", 1, 2**63 - 1, 2 << 20),
    ("bfs_prof_split", "bool", 0, 1, 0),
    ("merge_items", "bool", 0, 1, 1),
    ("merge_mode", "range", 0, 2, 0),
    ("dist_timing", "bool", 0, 1, 0),
    ("dist_collective", "range", 0, 1, 0),
    ("dist_force_self", "bool", 0, 1, 0),
    ("dist_test_delay_us", "range", 0, 100000, 0),
    ("transpose_mode", "range", 0, 3, 0),
    ("expand_compact", "bool", 0, 1, 1),
    ("pagerank_parts", "range", 0, 2, 1),
    ("expand_first_hop", "bool", 0, 1, 1),
    ("expand_xcd", "bool", 0, 1, 1),
    ("expand_xcd_relabel", "bool", 0, 1, 1),
    ("expand_xcd_min_mb", "range", 0, 1 << 20, 32),
    ("expand_xp_direct", "range", 0, 1, 1),
    ("expand_xp_fold", "range", 0, 1, 1),
    ("expand_xp_fold_min_words", "pow2", 2, 32, 8),
    ("expand_xp_dense", "range", 0, 1, 1),
    ("expand_scan_min", "range", 0, 2**31 - 1, 2048),
    ("expand_scan_rows", "pow2", 64, 4096, 1024),
    ("expand_scan_lanes", "range", 1, 16, 3),
    ("expand_records", "bool", 0, 1, 1),
    ("expand_nt", "range", 0, 7, 1),
    ("expand_emit_sort", "range", 0, 2, 1),
    ("pinned_results", "bool", 0, 1, 1),
    ("pinned_pool_mb", "range", 0, 1 << 20, 4096),
    ("wcc_mode", "range", 0, 2, 0),
    ("bc_batch", "range", 0, 64, 0),
    ("maxflow_global_every", "range", 0, 1 << 20, 0),
    ("bc_direction", "range", 0, 2, 0),
    ("expand_group_items", "range", 0, 1, 1),
    ("spdag_sides", "range", 0, 3, 0),
    ("expand_xp_lookahead", "range", 0, 1, 1),
    ("expand_xp_cut", "range", 0, 1, 1),
    ("expand_xp_stream_wgs", "range", 0, 65536, 0),
]

# read-only counters of fgpu_get_option (the table in ctx.hip); "msf_last_entries_round<k>" keeps its own parse
COUNTERS = [
    "dist_self_calls", "expand_kernel_launches", "bfs_cp_last_mask", "bfs_pb_last_levels", "expand_scan_last_live",
    "expand_scan_last_passes", "expand_xp_piece_folds", "expand_xp_slot_folds", "expand_xp_last_direct", "expand_xp_last_groups",
    "harmonic_last_entries", "harmonic_last_gathered", "sssp_last_delta_log2", "expand_xp_last_chunks", "expand_xp_last_shared_rows",
    "expand_group_item_launches",
]


def test_option_table_keeps_every_name_bound_and_default(tmp_path):
    """tests/host/options_check.cpp walks the table under the address and undefined-behaviour sanitizers, as a child process
    (nothing sanitized is loaded into this interpreter), and prints one line per row."""
    exe = str(tmp_path / "options_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "options_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(f) if f.lstrip("-").isdigit() else f for f in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(set(n for n, *_ in rows)), "a name appears twice in the table"
    assert sorted(rows) == sorted(OPTIONS)


def _quoted_names(comment):
    return set(re.findall(r'"([a-z][a-z0-9_]*)(?:<k>)?"', comment))


def test_header_documents_exactly_the_names_the_library_knows():
    hdr = open(os.path.join(ROOT, "include", "fgpu.h")).read()
    ctx_src = open(os.path.join(ROOT, "falkordb_amd", "csrc", "ctx.hip")).read()
    assert sorted(re.findall(r'FGPU_COUNTER\("([a-z0-9_]+)"', ctx_src)) == sorted(COUNTERS)
    above = {}
    for fn in ("fgpu_set_option", "fgpu_get_option"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*fgpu_info " + fn + r"\(", hdr, flags=re.S)
        assert m, f"no comment above {fn}"
        above[fn] = _quoted_names(m.group(1))
    settable = {n for n, *_ in OPTIONS} | {"transpose_wb", "sssp_delta_log2"}
    counters = set(COUNTERS) | {"msf_last_entries_round"}
    assert settable - above["fgpu_set_option"] == set(), "settable options the header does not list above fgpu_set_option"
    assert counters - above["fgpu_get_option"] == set(), "counters the header does not list above fgpu_get_option"
    known = settable | counters
    assert above["fgpu_set_option"] - known == set(), "names above fgpu_set_option that the library does not know"
    assert above["fgpu_get_option"] - known == set(), "names above fgpu_get_option that the library does not know"


def test_malformed_fgpu_opts_raises_before_any_library_call(monkeypatch):
    from falkordb_amd import _ffi, engine
    monkeypatch.setattr(_ffi, "load", lambda: pytest.fail("the library was loaded before FGPU_OPTS was parsed"))
    for bad in ("expand_mode", "expand_mode=1,tiled_u", "expand_mode=x", "=1"):
        monkeypatch.setenv("FGPU_OPTS", bad)
        with pytest.raises(ValueError) as e:
            engine.Context(0)
        assert repr(bad.split(",")[-1]) in str(e.value)


def _stub_context(values, refused=None):
    """An engine.Context that opens nothing: its options are a dict, every call is recorded, `refused` cannot be set."""
    from falkordb_amd import _ffi, engine

    class Stub(engine.Context):
        def __init__(self):
            self.values, self.calls = dict(values), []

        def get_option(self, name):
            self.calls.append(("get", name))
            return self.values[name]

        def set_option(self, name, value):
            self.calls.append(("set", name, value))
            if name == refused:
                raise _ffi.FgpuError(_ffi.FGPU_INVALID, f"{name} refused")
            self.values[name] = value

        def close(self):
            pass

    return Stub()


def test_options_guard_sets_in_order_and_restores_in_reverse():
    found = {"a": 1, "b": 2, "c": 3}
    ctx = _stub_context(found)
    with ctx.options(a=10, b=20, c=30):
        assert ctx.values == {"a": 10, "b": 20, "c": 30}
    assert ctx.values == found
    assert ctx.calls == [("get", "a"), ("set", "a", 10), ("get", "b"), ("set", "b", 20), ("get", "c"), ("set", "c", 30),
                         ("set", "c", 3), ("set", "b", 2), ("set", "a", 1)]


def test_options_guard_restores_when_the_body_raises():
    ctx = _stub_context({"a": 1, "b": 2})
    with pytest.raises(KeyError, match="from the body"):
        with ctx.options(a=10, b=20):
            assert ctx.values == {"a": 10, "b": 20}
            raise KeyError("from the body")
    assert ctx.values == {"a": 1, "b": 2}
    assert ctx.calls[-2:] == [("set", "b", 2), ("set", "a", 1)]


def test_options_guard_undoes_a_half_made_entry():
    from falkordb_amd._ffi import FGPU_INVALID, FgpuError
    ctx = _stub_context({"a": 1, "b": 2, "c": 3}, refused="b")
    entered = False
    with pytest.raises(FgpuError) as e:
        with ctx.options(a=10, b=20, c=30):
            entered = True
    assert e.value.code == FGPU_INVALID and not entered
    assert ctx.values == {"a": 1, "b": 2, "c": 3}
    # a is put back, b (never changed) is not set again, c is never read or set
    assert ctx.calls == [("get", "a"), ("set", "a", 10), ("get", "b"), ("set", "b", 20), ("set", "a", 1)]
