"""CPU: the graphs of tests/test_gpu_blocked.py still reach the paths of blocked.hip they were built for.

tests/blocked_layout.py restates the rules of blocked_build in numpy; here its plan is held to the unit counts the R-MAT
full passes are known to give, its padding to a matrix small enough to count by hand, and every case of make_case() to the
preconditions that make it worth a GPU run, at 256 and at 304 compute units: a later edit of a generator cannot silently
stop reaching a path."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blocked_layout as bl  # noqa: E402


def test_plan_restates_blocked_build():
    # the full passes at the benchmark's sizes: 512 units for a grid of 512 workgroups, windows of N / 256 rows
    assert bl.plan(1 << 22, 1 << 22, 256) == (14, 256, 16, 2, 8)
    assert bl.plan(1 << 24, 1 << 24, 256) == (16, 256, 64, 2, 32)
    assert bl.plan(1 << 26, 1 << 26, 256) == (17, 512, 256, 1, 256)
    # everything the suite ran before: one tile, one part, the smallest window
    for n in (1000, 1 << 10, 1 << 13, 1 << 16, 1 << 18):
        assert bl.plan(n, n, 256)[:1] + bl.plan(n, n, 256)[2:] == (10, 1, 1, 1), n
    # the window grows only past 256 windows and stops at 2^17 rows
    assert bl.plan(256 << 10, 1, 256)[0] == 10 and bl.plan((256 << 10) + 1024, 1, 256)[0] == 11
    assert bl.plan(1 << 30, 1, 256)[:2] == (17, 1 << 13)
    # nsplit doubles to reach two units per CU, never past ntiles, and is clamped to it
    assert bl.plan(1 << 10, 3 << 18, 256)[3:] == (3, 1)
    assert bl.plan(200 << 10, 64 << 18, 256)[3:] == (4, 16)
    assert bl.plan(200 << 10, 64 << 18, 304)[3:] == (4, 16)
    assert bl.plan(100 << 10, 64 << 18, 304)[3:] == (8, 8)


def test_padded_entries_by_hand():
    # n = 3000: wbits 10, three windows, one tile.  Window 0: row 0 with 5 entries, row 32 with 2 (one bucket: 7 -> 8), row 1
    # with 1 (-> 4): 12 -> 256.  Window 1: row 1024 with 256 entries: 256, no pad.  Window 2: row 2048 with 256 and row 2049
    # with 1: 260 -> 512.
    rows = [0] * 5 + [32] * 2 + [1] + [1024] * 256 + [2048] * 256 + [2049]
    cols = list(range(5)) + [7, 9] + [11] + list(range(256)) + list(range(256)) + [3]
    m = oracle.build_csr(3000, 3000, np.array(rows, dtype=np.uint64), np.array(cols, dtype=np.uint64))
    assert bl.plan(3000, 3000, 256) == (10, 3, 1, 1, 1)
    assert bl.padded_entries(m, 10) == (256 + 256 + 512, 3, 3)
    cnt = bl.bucket_counts(m, 10)
    assert cnt[0, 0] == 7 and cnt[0, 1] == 1 and cnt[1, 0] == 256 and cnt[2].tolist()[:2] == [256, 1]
    assert bl.padded_entries(oracle.empty(3000, 3000), 10) == (0, 0, 3)


def test_unit_profile_names_every_kind_of_hole():
    ne = np.zeros((3, 7), dtype=bool)
    ne[0, [2, 5]] = True          # parts of 3 tiles: [0, 3) lead 2; [3, 6) lead 2; [6, 7) dead
    ne[1, [0, 2, 3]] = True       # [0, 3) mid 1; [3, 6) trail 2; [6, 7) dead
    u = bl.unit_profile(ne, 4, 3)  # (a fourth part lies past the 7 tiles)
    assert [x["kind"] for x in u] == ["live", "live", "dead", "past"] * 2 + ["idle", "idle", "idle", "past"]
    assert [(x["lead"], x["mid"], x["trail"]) for x in u[:2]] == [(2, 0, 0), (2, 0, 0)]
    assert [(x["lead"], x["mid"], x["trail"]) for x in u[4:6]] == [(0, 1, 0), (0, 0, 2)]


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("name", list(bl.CASES))
def test_case_reaches_its_paths(name, cus):
    case = bl.make_case(name)
    assert case.n == bl.CASES[name] and case.M.nrows == case.M.ncols == case.n
    fig = bl.check_preconditions(case, cus)
    print(name, cus, fig)
    wbits, nwindows, ntiles, _, _ = fig["plan"]
    total, nonempty, nblocks = bl.padded_entries(case.M, wbits)
    assert nblocks == nwindows * ntiles and total % bl.CHUNK == 0 and case.M.nnz < total <= nonempty * 2 ** 14


@pytest.mark.parametrize("name", list(bl.CASES))
def test_case_frontiers_against_the_oracle(name):
    """A one-bit frontier gives exactly the rows that store that column, and the case's bitmaps are the oracle's own."""
    case = bl.make_case(name)
    n = case.n
    rows, cols = case.M.pairs()
    for key, col in case.special["cols"].items():
        want = oracle.vxm(case.a, oracle.bits_from_ids(n, [col]), None)
        stored = np.unique(rows[cols == np.uint64(col)])
        np.testing.assert_array_equal(oracle.ids_from_bits(want, n), stored, err_msg=key)
        np.testing.assert_array_equal(case.rows_storing(col), stored, err_msg=key)
    ids = np.array([0, 5, 63, 64, n - 1])
    np.testing.assert_array_equal(bl.bits(n, ids), oracle.bits_from_ids(n, ids))
    names = [k for k, _ in case.frontiers()]
    assert names == ["last_tile", "empty_tile", "fifth", "full"]
    full = dict(case.frontiers())["full"]
    has_entry = np.nonzero(np.diff(case.M.rowptr.astype(np.int64)))[0].astype(np.uint64)
    np.testing.assert_array_equal(oracle.ids_from_bits(oracle.vxm(case.a, full, None), n), has_entry)
    mk = case.mask()
    assert abs(len(oracle.ids_from_bits(mk, n)) - n // 3) <= 1
    np.testing.assert_array_equal(oracle.vxm(case.a, full, mk), oracle.vxm(case.a, full, None) & ~mk)
