"""GPU: fgpu_harmonic (algo.HarmonicCentrality's LAGr_HarmonicCentrality core, HyperBall) against the numpy checker of
tests/hc_check.py.  Every case is compared in the same four ways: the final sketches by array equality, the stats by equality,
reachable by equality (after asserting that no final estimate sits within 1e-6 of a rounding point), the score within 1e-9
absolute — S is exact, so an estimate differs between two libm `log`s by a few ulp of a value <= ~1e4 (about 1e-12), and a
score is a sum of at most a few hundred such differences divided by t."""
import os
import sys
import threading

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hc_check import csr_of, harmonic, round_margin  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_want = {}                                                                  # the checker's answers, computed once per graph


def up(ctx, n, rows, cols):
    rp, ci = csr_of(n, rows, cols)
    A = ctx.mat_from_coo(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))
    return A, rp, ci


def bitmap(act):
    """bool[n] -> the nrows-bit LSB-first u64 words fgpu_harmonic takes"""
    n = len(act)
    bits = np.zeros((n + 63) // 64 * 64, dtype=bool)
    bits[:n] = act
    return np.packbits(bits, bitorder="little").view(np.uint64)


def hypersparse(ctx, m):
    """The same entries stored as a delta layer stores them: the ids of the non-empty rows + a row-pointer array over those."""
    rp, ci, _ = m.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    return ctx.mat_from_csr(m.nrows, m.ncols, short, ci, hyper_rows=rows)


def expect(key, n, rp, ci, active=None):
    if key not in _want:
        margin = round_margin(n, rp, ci, active)
        _want[key] = harmonic(n, rp, ci, active) + (margin,)
    return _want[key]


def check(ctx, A, key, n, rp, ci, active=None):
    ws, wr, wc, wst, margin = expect(key, n, rp, ci, active)
    assert margin > 1e-6, margin                                           # llround cannot flip on a few ulp
    score, reach, regs, st = engine.harmonic(ctx, A, bitmap(active) if active is not None else None, stats=True, registers=True)
    assert np.array_equal(regs, wc), np.flatnonzero((regs != wc).any(axis=1))[:10]
    assert st == wst, (st, wst)
    assert np.array_equal(reach, wr), np.flatnonzero(reach != wr)[:10]
    err = float(np.abs(score - ws).max()) if n else 0.0
    print(key, "n", n, "stats", st, "round margin", margin, "largest score difference", err)
    assert err <= 1e-9
    if active is not None:
        off = ~np.asarray(active, dtype=bool)
        assert (score[off] == 0.0).all() and (reach[off] == -1).all() and not regs[off].any()
    return score, reach, st


def run(ctx, key, n, rows, cols, active=None):
    A, rp, ci = up(ctx, n, rows, cols)
    return check(ctx, A, key, n, rp, ci, active)


def random_graph():
    rng = np.random.default_rng(4099)
    n = 4099
    return n, rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)


def skewed_graph():
    """cubic skew: a few rows and columns take most of the 6000 entries; duplicate (row, col) pairs included"""
    rng = np.random.default_rng(1000)
    n = 1000
    rows = (n * rng.random(6000) ** 3).astype(np.int64)
    cols = (n * rng.random(6000) ** 3).astype(np.int64)
    return n, rows, cols


def star_graph():
    n = 5001
    leaves = np.arange(1, n)
    hub = np.zeros(n - 1, dtype=np.int64)
    return n, np.concatenate([hub, leaves]), np.concatenate([leaves, hub])


def test_empty_and_single_vertex(ctx):
    A = ctx.mat_new(0, 0)
    score, reach, regs, st = engine.harmonic(ctx, A, stats=True, registers=True)
    assert len(score) == 0 and len(reach) == 0 and regs.shape == (0, 1024) and st == [0, 0, 0, 0]
    one = ctx.mat_new(1, 1)
    rp, ci = csr_of(1, [], [])
    score, reach, st = check(ctx, one, "one", 1, rp, ci)
    assert score.tolist() == [0.0] and reach.tolist() == [0] and st == [0, 0, 0, 0]
    score, reach, st = run(ctx, "loop", 1, [0], [0])
    assert score.tolist() == [0.0] and reach.tolist() == [0] and st == [0, 0, 0, 0]


def test_directed_path_of_300(ctx):
    # close to 299 dependent iterations: the batched read-back, and the skip rule (one sketch per iteration stops changing)
    n = 300
    score, reach, st = run(ctx, "path300", n, np.arange(n - 1), np.arange(1, n))
    assert 200 < st[0] <= n - 1                                            # at most the diameter; a few register collisions less
    assert score[n - 1] == 0.0 and reach[n - 1] == 0
    assert score[0] > score[n - 2] > 0.0


def test_cycle_of_67(ctx):
    n = 67
    score, reach, st = run(ctx, "cycle67", n, np.arange(n), (np.arange(n) + 1) % n)
    assert st[0] <= n - 1 and st[3] == n
    assert np.abs(reach - 66).max() <= 3 * 1.04 / 32 * 67                  # everyone reaches the 66 others: three standard errors


def flow_cases():
    import json
    return json.load(open(os.path.join(ROOT, "tests", "golden", "harmonic_flow.json")))["cases"]


@pytest.mark.parametrize("case", flow_cases(), ids=[c["name"] for c in flow_cases()])
def test_flow_fixtures(ctx, case):
    names = [nd["name"] for nd in case["nodes"]]
    at = {name: k for k, name in enumerate(names)}
    rows = [at[e[0]] for e in case["edges"]]
    cols = [at[e[2]] for e in case["edges"]]
    score, reach, st = run(ctx, "flow_" + case["name"], len(names), rows, cols)
    q = case["queries"][0]
    if not q["labels"] and not q["types"]:                                 # the unfiltered relations hold on the plain matrix
        for a, b in q["greater"]:
            assert score[at[a]] > score[at[b]]
        for z in q["zeros"]:
            assert score[at[z]] == 0.0
        if "top" in q:
            assert int(np.argmax(score)) == at[q["top"]]


def test_star_with_a_hub_row_takes_the_hub_path_and_the_raw_estimator(ctx):
    n, rows, cols = star_graph()
    A, rp, ci = up(ctx, n, rows, cols)
    assert np.diff(rp).max() == 5000                                       # a hub row: two chunks and the fold
    score, reach, st = check(ctx, A, "star5000", n, rp, ci)
    assert st[0] == 2
    assert reach[0] + 1 > 2560                                             # the estimate left the small-range correction


def test_random_graph_on_both_sides_of_the_estimator_switch(ctx):
    n, rows, cols = random_graph()
    score, reach, st = run(ctx, "random4099", n, rows, cols)
    assert (reach + 1 <= 2560).any() and (reach + 1 > 2560).any()


def test_skewed_graph_with_duplicate_pairs(ctx):
    n, rows, cols = skewed_graph()
    assert len(set(zip(rows.tolist(), cols.tolist()))) < len(rows)         # duplicates are given to the builder
    run(ctx, "skewed1000", n, rows, cols)


@pytest.mark.parametrize("which", ["random", "skewed"])
def test_active_bitmap_induced_subgraph(ctx, which):
    n, rows, cols = random_graph() if which == "random" else skewed_graph()
    active = np.random.default_rng(60).random(n) < 0.6
    run(ctx, which + "_active", n, rows, cols, active)


def test_hypersparse_input(ctx):
    n, rows, cols = random_graph()
    A, rp, ci = up(ctx, n, rows, cols)
    check(ctx, hypersparse(ctx, A), "random4099", n, rp, ci)


def test_repeats_are_bit_identical_and_a_pinned_out_is_filled(ctx):
    n, rows, cols = skewed_graph()
    A, rp, ci = up(ctx, n, rows, cols)
    a = engine.harmonic(ctx, A, registers=True)
    b = engine.harmonic(ctx, A, registers=True)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    pinned = (ctx.host_array(n, np.float64), ctx.host_array(n, np.int64))
    c = engine.harmonic(ctx, A, out=pinned)
    assert c[0] is pinned[0] and c[1] is pinned[1] and c[2] is None and c[3] is None
    assert c[0].tobytes() == a[0].tobytes() and np.array_equal(c[1], a[1])


def test_two_threads_on_one_context(ctx):
    n, rows, cols = skewed_graph()
    A, rp, ci = up(ctx, n, rows, cols)
    sn, srows, scols = star_graph()
    S, _, _ = up(ctx, sn, srows, scols)
    want = {"a": engine.harmonic(ctx, A, registers=True, stats=True), "s": engine.harmonic(ctx, S, registers=True, stats=True)}
    errors = []

    def work(key, m):
        try:
            for _ in range(3):
                got = engine.harmonic(ctx, m, registers=True, stats=True)
                assert got[0].tobytes() == want[key][0].tobytes() and np.array_equal(got[1], want[key][1])
                assert np.array_equal(got[2], want[key][2]) and got[3] == want[key][3]
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=("a", A)), threading.Thread(target=work, args=("s", S))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_error_codes(ctx):
    import ctypes as C
    A = ctx.mat_rmat(8, 4, 3)
    rect = ctx.mat_new(4, 5)
    before = ctx.device_bytes()
    with pytest.raises(FgpuError) as e:
        engine.harmonic(ctx, rect)
    assert e.value.code == -6                                          # FGPU_DIM_MISMATCH
    score = np.zeros(A.nrows, dtype=np.float64)
    reach = np.zeros(A.nrows, dtype=np.int64)
    dp, ip = score.ctypes.data_as(C.POINTER(C.c_double)), reach.ctypes.data_as(engine.i64p)
    assert ctx.lib.fgpu_harmonic(ctx._h, A._h, None, None, ip, None, None) == -2      # FGPU_NULL_POINTER
    assert ctx.lib.fgpu_harmonic(ctx._h, A._h, None, dp, None, None, None) == -2
    assert ctx.lib.fgpu_harmonic(ctx._h, None, None, dp, ip, None, None) == -2
    assert ctx.lib.fgpu_harmonic(None, A._h, None, dp, ip, None, None) == -2
    assert ctx.device_bytes() == before
    engine.harmonic(ctx, A, out=(score, reach))                        # the context still works
    assert ctx.get_option("harmonic_last_gathered") > 0
    assert ctx.get_option("harmonic_last_entries") >= ctx.get_option("harmonic_last_gathered")
