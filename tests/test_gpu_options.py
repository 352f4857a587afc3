"""GPU: fgpu_set_option / fgpu_get_option on a live context — every settable option reads back, a refused value changes nothing,
counters cannot be set.  The table itself is walked on the host (tests/test_options_cpu.py); this is the path through the library."""
import pytest

from falkordb_amd._ffi import FGPU_INVALID, FgpuError

pytestmark = pytest.mark.gpu


def _invalid(call, *args):
    with pytest.raises(FgpuError) as e:
        call(*args)
    assert e.value.code == FGPU_INVALID
    return str(e.value)


# (name, legal values, a value that is refused).  expand_records is a 0 / not 0 option: no value is refused, 7 is stored as 1.
# tiled_wgs could be set but not read before the option table.
@pytest.mark.parametrize("name,legal,illegal", [
    ("expand_mode", (0, 1), 3),
    ("tiled_u", (8, 4), 3),
    ("expand_records", (0, 1), None),
    ("bfs_pb_min_edges", (2 << 20, 1 << 40), 0),
    ("tiled_wgs", (0, 7), 65537),
    ("spdag_sides", (0, 3), 4),
    ("expand_xp_stream_wgs", (0, 7), 65537),
    ("expand_group_items", (1, 0), 2),
])
def test_set_get_reject_restore(ctx, name, legal, illegal):
    found = ctx.get_option(name)
    try:
        other = next(v for v in legal if v != found)
        ctx.set_option(name, other)
        assert ctx.get_option(name) == other
        if illegal is None:
            ctx.set_option(name, 7)
            assert ctx.get_option(name) == 1
        else:
            assert name in _invalid(ctx.set_option, name, illegal)
            assert ctx.get_option(name) == other
    finally:
        ctx.set_option(name, found)
    assert ctx.get_option(name) == found


def test_unknown_names_counters_and_special_cases(ctx):
    assert "no_such_option" in _invalid(ctx.set_option, "no_such_option", 1)
    assert "no_such_option" in _invalid(ctx.get_option, "no_such_option")
    assert ctx.get_option("expand_kernel_launches") >= 0
    _invalid(ctx.set_option, "expand_kernel_launches", 0)
    for name in ("expand_xp_last_chunks", "expand_xp_last_shared_rows", "expand_group_item_launches"):
        assert ctx.get_option(name) >= 0
        _invalid(ctx.set_option, name, 0)
    ctx.get_option("sssp_last_delta_log2")       # an exponent: any sign
    _invalid(ctx.set_option, "sssp_last_delta_log2", 0)
    assert ctx.get_option("msf_last_entries_round3") >= 0
    _invalid(ctx.get_option, "msf_last_entries_round32")
    _invalid(ctx.get_option, "transpose_wb")     # process-wide, no stored value to read
    ctx.set_option("transpose_wb", 0)            # 0 = pick: the default
