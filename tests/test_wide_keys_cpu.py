"""The case builders of tests/wide_keys.py hold what they claim (no GPU needed): every group of a width's key set is present and
below the key space, the cases keep the stability probe and their duplicates, and the references are recomputed here with
Python sets and dicts."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_keys as wk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_ladder_is_the_one_the_plan_check_pins():
    assert wk.LADDER == (2 ** 22, 2 ** 24 + 1, 2 ** 26, 2 ** 26 + 1, 2 ** 27, 2 ** 27 + 1)
    assert [wk.key_bits(n) for n in wk.LADDER] == [22, 25, 26, 27, 27, 28]
    assert [wk.staged_levels(n) for n in wk.LADDER] == [3, 3, 3, 3, 3, 4]
    assert [n <= wk.TWO_LEVEL_MAX for n in wk.LADDER] == [True, True, True, False, False, False]
    assert sum(1 for n in wk.LADDER if n & (n - 1)) == 3            # three partial last buckets / segments
    # the constants the builders restate
    text = open(os.path.join(ROOT, "falkordb_amd", "csrc", "sort_plan.hpp")).read()
    assert int(re.search(r"KS_MAX_BUCKETS = (\d+);", text).group(1)) << int(re.search(r"KS_MAX_WB = (\d+);", text).group(1)) \
        == wk.TWO_LEVEL_MAX
    assert "(kb + 8) / 9" in text and "kb >= 17 && L < 3" in text


@pytest.mark.parametrize("nkeys", wk.LADDER)
def test_key_set_groups(nkeys):
    g = wk.key_groups(nkeys)
    keys = wk.key_set(nkeys)
    kb = wk.key_bits(nkeys)
    assert len(keys) == wk.NKEYS_ENTRIES >= 4097 and keys.dtype == np.uint64
    assert int(keys.max()) == nkeys - 1 and int(keys.min()) == 0
    have = set(keys.tolist())
    assert set(range(64)) <= have and set(range(nkeys - 64, nkeys)) <= have
    for j in range(kb):
        assert {(1 << j) - 1, 1 << j, nkeys - 1 - (1 << j)} <= have, j
    assert len(g["bits"]) == 3 * kb and (1 << (kb - 1)) < nkeys <= (1 << kb)
    hk = wk.heavy_key(nkeys)
    assert (keys == hk).sum() == wk.HEAVY == 300
    hs = wk.heavy_slice(nkeys)
    assert (keys[hs] == hk).all()
    assert wk.narrow_ids(nkeys)[hs].tolist() == list(range(300))
    assert len(g["random"]) > 4000 and len(set(g["random"].tolist())) > 3900
    assert int(wk.narrow_ids(nkeys).max()) == wk.NARROW - 1
    assert wk.key_set(nkeys) is not keys and np.array_equal(wk.key_set(nkeys), keys)   # deterministic


@pytest.mark.parametrize("nkeys", wk.LADDER)
def test_transpose_case(nkeys):
    t = wk.transpose_case(nkeys)
    assert t is wk.transpose_case(nkeys)                           # cached
    n = len(t["colidx"])
    assert 4097 <= n <= wk.NKEYS_ENTRIES and int(t["rowptr"][-1]) == n and len(t["rowptr"]) == wk.NARROW + 1
    coords = list(zip(t["rows"].tolist(), t["cols"].tolist()))
    assert coords == sorted(set(zip(wk.narrow_ids(nkeys).tolist(), wk.key_set(nkeys).tolist())))
    for r in range(wk.NARROW):                                     # a sorted-unique CSR
        row = t["colidx"][int(t["rowptr"][r]):int(t["rowptr"][r + 1])]
        assert (np.diff(row.astype(np.int64)) > 0).all()
    back = list(zip(t["t_rows"].tolist(), t["t_cols"].tolist()))
    assert back == sorted((c, r) for r, c in coords)
    hk = wk.heavy_key(nkeys)
    assert [c for r, c in back if r == hk] == list(range(300))     # the stability probe: one key, values ascending
    assert len(set(t["vals"].tolist())) == n
    vd = dict(zip(coords, t["vals"].tolist()))
    assert t["t_vals"].tolist() == [vd[(c, r)] for r, c in back]


@pytest.mark.parametrize("shape", wk.COO_SHAPES)
@pytest.mark.parametrize("nkeys", wk.LADDER)
def test_coo_case(nkeys, shape):
    c = wk.coo_case(nkeys, shape)
    assert (c["nrows"], c["ncols"]) == {"tall": (nkeys, 300), "wide": (300, nkeys), "square": (nkeys, nkeys)}[shape]
    r, cc, v = c["rows"].tolist(), c["cols"].tolist(), c["vals"].tolist()
    assert len(r) == len(cc) == len(v) == 5700 >= 4096 and len(set(v)) == len(v)
    assert max(r) == c["nrows"] - 1 and max(cc) == c["ncols"] - 1 and min(r) == 0 and min(cc) == 0
    want = {}
    for k in zip(r, cc, v):
        want[k[:2]] = k[2]
    assert 4097 <= len(want) <= len(r) - 600                       # duplicates are there
    ref = list(zip(c["ref_rows"].tolist(), c["ref_cols"].tolist()))
    assert ref == sorted(want) and c["ref_vals"].tolist() == [want[k] for k in ref]
    firsts = {}
    for k in zip(r, cc, v):
        firsts.setdefault(k[:2], k[2])
    assert sum(1 for k in want if want[k] != firsts[k]) >= 600      # "last wins" differs from "first wins"
    assert list(zip(r, cc)) != sorted(zip(r, cc))                  # shuffled


@pytest.mark.parametrize("side", wk.EDGE_SIDES)
@pytest.mark.parametrize("nkeys", wk.LADDER)
def test_edges_case(nkeys, side):
    e = wk.edges_case(nkeys, side)
    assert (e["nrows"], e["ncols"]) == ((nkeys, 300) if side == "rows" else (300, nkeys))
    triples = list(zip(e["srcs"].tolist(), e["dsts"].tolist(), e["ids"].tolist()))
    assert len(triples) == 5700 and len(set(triples)) == 5700 and len({t[2] for t in triples}) == 5700
    pairs = {}
    for s, d, i in triples:
        pairs.setdefault((s, d), set()).add(i)
    order = sorted(pairs)
    assert list(zip(e["fwd_rows"].tolist(), e["fwd_cols"].tolist())) == order
    assert e["fwd_vals"].tolist() == [min(pairs[p]) if len(pairs[p]) == 1 else wk.MULTI for p in order]
    assert list(zip(e["bwd_rows"].tolist(), e["bwd_cols"].tolist())) == sorted((d, s) for s, d in order)
    multi = [p for p in order if len(pairs[p]) > 1]
    assert len(multi) >= 600 and e["multi_key"].tolist() == [(s << 32) | d for s, d in multi]
    assert np.diff(e["multi_off"].astype(np.int64)).tolist() == [len(pairs[p]) for p in multi]
    assert e["multi_ids"].tolist() == [i for p in multi for i in sorted(pairs[p])]


def test_probe_coords():
    pr, pc, exp = wk.probe_coords([0, 0, 5], [0, 1, 9])
    assert pc.tolist() == [0, 1, 9, 2 ** 64 - 1, 0, 8, 1, 2, 10] and pr.tolist() == [0, 0, 5] * 3
    assert exp.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("N", [2 ** 31 + 5, 2 ** 32 - 2])
def test_straddle_contents(N):
    x, y, z = (wk.straddle_rows(N, s) for s in (0, 1, 2))
    sx, sy, sz = wk.as_set(x), wk.as_set(y), wk.as_set(z)
    for m in wk.marks(N):
        assert any(m in cols for cols in x.values())
    assert wk.marks(N) == [0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, N - 2, N - 1] and len(set(wk.marks(N))) == 6
    run = wk.run_across(N)
    assert run[0] < 2 ** 31 - 1 and run[-1] > 2 ** 31 and all(b - a == 1 for a, b in zip(run, run[1:])) and run[-1] < N
    assert set(run) <= set(x[1]) and len(run) >= 70                # more than one wavefront of a row
    assert {0, 63, 64, 65, wk.WIDE_ROWS - 1} <= set(x) and max(x) == wk.WIDE_ROWS - 1
    for s in (sx, sy, sz):
        assert all(r < wk.WIDE_ROWS and c < N for r, c in s)
        assert any(c >= 2 ** 31 for _, c in s) and any(c < 2 ** 31 for _, c in s)
    assert sx & sy and sx - sy and sy - sx and sx & sz and sy & sz and sy - sz
    assert any(c >= 2 ** 31 for _, c in sx & sy) and any(c < 2 ** 31 for _, c in sx & sy)
    for rows in (x, y, z):
        rp, ci = wk.dense_arrays(wk.WIDE_ROWS, rows)
        hrp, hci, hr = wk.hyper_arrays(rows)
        assert int(rp[-1]) == len(ci) == len(wk.as_set(rows)) == int(hrp[-1]) and np.array_equal(ci, hci)
        assert hr.tolist() == sorted(rows) and len(rp) == wk.WIDE_ROWS + 1
        got = {(r, int(c)) for r in range(wk.WIDE_ROWS) for c in ci[int(rp[r]):int(rp[r + 1])]}
        assert got == wk.as_set(rows)
    assert wk.merged(sx, sy, sz) == (sx - sz) | sy and wk.merged(sx, sy, sz, True) == (sx - sz) | (sy - sz)
    assert wk.merged(sx, sy, sz) != wk.merged(sx, sy, sz, True)


def test_tall_rows():
    t = wk.tall_rows()
    assert wk.TALL_NROWS == 2 ** 32 - 2 and sorted(t) == wk.marks(wk.TALL_NROWS)
    assert all(len(c) == 3 and max(c) < 1000 for c in t.values())
    assert wk.as_set(wk.tall_rows(1)) & wk.as_set(t) and wk.as_set(wk.tall_rows(1)) - wk.as_set(t)
