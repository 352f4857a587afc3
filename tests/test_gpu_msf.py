"""GPU: fgpu_msf (algo.MSF's LAGraph_msf core) against the Kruskal checker of tests/msf_check.py.  The edge order is strict and
total, so the forest is unique: every comparison is array equality of component, rows, cols and the weight BITS."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_check import bits_of, components, msf  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


def bitmap(act):
    n = len(act)
    bits = np.zeros((n + 63) // 64 * 64, dtype=bool)
    bits[:n] = act
    return np.packbits(bits, bitorder="little").view(np.uint64)


def random_pairs(rng, n, m, lo=0, hi=None):
    """m distinct pairs (a < b) with both ends in [lo, hi)"""
    hi = n if hi is None else hi
    a = rng.integers(lo, hi, 3 * m + 8)
    b = rng.integers(lo, hi, 3 * m + 8)
    keep = a != b
    a, b = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    key = np.unique(a.astype(np.int64) * n + b)
    key = rng.permutation(key)[:m]
    return key // n, key % n


def sym(lo, hi, bits=None, loops=()):
    """both directions of every pair (+ diagonal entries `loops`), with the same bits on both"""
    loops = np.asarray(loops, dtype=np.int64)
    rows = np.concatenate([lo, hi, loops]).astype(np.int64)
    cols = np.concatenate([hi, lo, loops]).astype(np.int64)
    if bits is None:
        return rows, cols, None
    return rows, cols, np.concatenate([bits, bits, np.full(len(loops), bits_of([-7.0])[0], dtype=U64)])


def upload(ctx, n, rows, cols, bits):
    return ctx.mat_from_coo(n, n, rows.astype(U64), cols.astype(U64), bits)


def check(ctx, n, rows, cols, bits, active=None, W=None):
    """run fgpu_msf on the symmetric entries and compare everything with the checker; returns (stats, result)"""
    if W is None:
        W = upload(ctx, n, rows, cols, bits)
    fr, fc, fb, comp = msf(n, rows, cols, bits, active)
    act = bitmap(active) if active is not None else None
    got = engine.msf(ctx, W, act, stats=True)
    gcomp, grows, gcols, gw, st = got
    assert np.array_equal(gcomp, comp)
    assert np.array_equal(grows, fr) and np.array_equal(gcols, fc)
    assert np.array_equal(gw.view(U64), fb)
    nact = n if active is None else int(np.count_nonzero(active))
    assert st[1] == len(fr) == nact - components(comp)
    assert st[3] == components(comp)
    return st, got


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_no_entries_and_one_edge(ctx, n):
    empty = np.zeros(0, dtype=np.int64)
    st, got = check(ctx, n, empty, empty, np.zeros(0, dtype=U64))
    assert st[0] == 0 and len(got[1]) == 0
    if n >= 2:
        rows, cols, bits = sym(np.array([0]), np.array([n - 1]), bits_of([2.5]))
        st, got = check(ctx, n, rows, cols, bits)
        assert st[0] == 1 and got[1].tolist() == [0] and got[2].tolist() == [n - 1] and got[3].tolist() == [2.5]


def test_path_with_increasing_weights_is_one_round(ctx):
    n = 5000
    lo = np.arange(n - 1)
    rows, cols, bits = sym(lo, lo + 1, bits_of(np.arange(1, n, dtype=np.float64)))
    st, _ = check(ctx, n, rows, cols, bits)
    assert st[0] == 1   # every vertex picks the edge towards vertex 0: hook chains thousands deep, one compress


def test_path_with_ruler_weights_takes_log_rounds(ctx):
    n = 4097
    lo = np.arange(n - 1)
    i = lo + 1
    tz = np.array([(int(x) & -int(x)).bit_length() - 1 for x in i], dtype=np.float64)
    rows, cols, bits = sym(lo, lo + 1, bits_of(tz))
    st, _ = check(ctx, n, rows, cols, bits)
    assert 10 <= st[0] <= 14


def test_random_graph_distinct_weights_ties_and_bool(ctx):
    rng = np.random.default_rng(11)
    n, m = 3000, 12000
    lo, hi = random_pairs(rng, n, m)
    rows, cols, bits = sym(lo, hi, bits_of(rng.permutation(m).astype(np.float64) * 0.37 - 500.0))
    check(ctx, n, rows, cols, bits)
    rows, cols, ones = sym(lo, hi, bits_of(np.ones(m)))
    _, a = check(ctx, n, rows, cols, ones)
    W = ctx.mat_from_coo(n, n, rows.astype(U64), cols.astype(U64))
    _, b = check(ctx, n, rows, cols, None, W=W)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)


SPECIAL = np.array([0x8000000000000000, 0x0, 0x7FF0000000000000, 0xFFF0000000000000, 0xC00C000000000000, 0xBFF0000000000000,
                    0x1, 0x3FF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF],
                   dtype=U64)


def test_special_values_and_their_negation(ctx):
    rng = np.random.default_rng(12)
    n, m = 500, 2500
    lo, hi = random_pairs(rng, n, m)
    b = SPECIAL[rng.integers(0, len(SPECIAL), m)]
    rows, cols, bits = sym(lo, hi, b)
    check(ctx, n, rows, cols, bits)
    rows, cols, bits = sym(lo, hi, b ^ U64(0x8000000000000000))   # the maximise form: every weight negated
    check(ctx, n, rows, cols, bits)


@pytest.mark.parametrize("hub_ties", [False, True], ids=["hub-distinct", "hub-all-equal"])
def test_hub_row_is_split_by_chunks(ctx, hub_ties):
    rng = np.random.default_rng(13)
    n, leaves = 6000, 5000
    slo, shi = np.zeros(leaves, dtype=np.int64) + 17, np.arange(100, 100 + leaves)   # the hub is vertex 17
    lo, hi = random_pairs(rng, n, 3000, 100, 100 + leaves)
    w_star = np.full(leaves, 4.0) if hub_ties else rng.permutation(leaves).astype(np.float64)
    w_rest = rng.integers(0, 8, 3000).astype(np.float64)
    plo = np.concatenate([np.minimum(slo, shi), lo])
    phi = np.concatenate([np.maximum(slo, shi), hi])
    rows, cols, bits = sym(plo, phi, bits_of(np.concatenate([w_star, w_rest])))
    assert np.bincount(rows, minlength=n)[17] >= 4096
    check(ctx, n, rows, cols, bits)
    if hub_ties:
        W = ctx.mat_from_coo(n, n, rows.astype(U64), cols.astype(U64))
        check(ctx, n, rows, cols, None, W=W)


def twelve_components(rng):
    """twelve components of unequal size, 40 isolated vertices, self-loops; n = 1037"""
    n = 1037
    ids = rng.permutation(n)
    iso, rest = ids[:40], ids[40:]
    cuts = np.sort(rng.choice(np.arange(5, len(rest) - 5), 11, replace=False))
    los, his = [], []
    for part in np.split(rest, cuts):
        k = len(part)
        t = np.arange(1, k)
        a, b = part[t], part[(t - 1) // 2]                 # a spanning tree keeps the part connected
        xa, xb = part[rng.integers(0, k, 2 * k)], part[rng.integers(0, k, 2 * k)]
        a, b = np.concatenate([a, xa]), np.concatenate([b, xb])
        los.append(np.minimum(a, b))
        his.append(np.maximum(a, b))
    lo, hi = np.concatenate(los), np.concatenate(his)
    keep = lo != hi
    key = np.unique(lo[keep].astype(np.int64) * n + hi[keep])
    lo, hi = key // n, key % n
    w = rng.integers(0, 6, len(lo)).astype(np.float64)
    loops = np.concatenate([iso[:10], rest[:30]])
    return n, sym(lo, hi, bits_of(w), loops)


def test_components_isolated_vertices_and_self_loops(ctx):
    n, (rows, cols, bits) = twelve_components(np.random.default_rng(14))
    st, got = check(ctx, n, rows, cols, bits)
    assert st[3] == 12 + 40


def test_active_bitmap_with_a_partial_last_word(ctx):
    n, (rows, cols, bits) = twelve_components(np.random.default_rng(15))
    active = np.ones(n, dtype=bool)
    active[::3] = False
    _, got = check(ctx, n, rows, cols, bits, active)
    comp, fr, fc = got[0], got[1].astype(np.int64), got[2].astype(np.int64)
    assert np.all(comp[~active] == -1) and np.all(comp[active] >= 0)
    assert np.all(active[fr]) and np.all(active[fc])
    # the induced subgraph on compact ids gives the same forest
    idx = np.cumsum(active) - 1
    keep = active[rows] & active[cols]
    ir, ic, _, _ = msf(int(active.sum()), idx[rows[keep]], idx[cols[keep]], bits[keep])
    assert np.array_equal(idx[fr], ir.astype(np.int64)) and np.array_equal(idx[fc], ic.astype(np.int64))


def test_hypersparse_snapshot(ctx):
    n, (rows, cols, bits) = twelve_components(np.random.default_rng(14))
    W = upload(ctx, n, rows, cols, bits)
    rp, ci, vv = W.export_csr()
    deg = np.diff(rp.astype(np.int64))
    hr = np.nonzero(deg)[0].astype(U64)
    short = np.concatenate([[0], np.cumsum(deg[deg > 0])]).astype(U64)
    H = ctx.mat_from_csr(n, n, short, ci, vals=vv, hyper_rows=hr)
    check(ctx, n, rows, cols, bits, W=H)
    HB = ctx.mat_from_csr(n, n, short, ci, hyper_rows=hr)
    check(ctx, n, rows, cols, None, W=HB)


def test_repeatable_equals_wcc_and_fills_a_host_array(ctx):
    rng = np.random.default_rng(16)
    n, m = 3000, 5000
    lo, hi = random_pairs(rng, n, m)
    rows, cols, bits = sym(lo, hi, bits_of(rng.integers(0, 4, m).astype(np.float64)))
    W = upload(ctx, n, rows, cols, bits)
    a = engine.msf(ctx, W, stats=True)
    b = engine.msf(ctx, W, stats=True)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]
    wc, _ = engine.wcc(ctx, W, None)
    assert np.array_equal(a[0], wc)
    out = ctx.host_array(n, np.int64)
    out[:] = -5
    c = engine.msf(ctx, W, out=out)
    assert c[0] is out and np.array_equal(out, a[0])


# the read-out of the sorted forest (csr_edge_list): k = 1, 256 and 257 pairs are one thread, exactly one workgroup of the
# emit kernel, and one element into the second
def weighted_path(n):
    """the path 0 - 1 - ... - (n-1); the weights (i * 37) % (n - 1) + 0.5 are distinct: 37 is coprime to 1, 256 and 257"""
    lo = np.arange(n - 1)
    return lo, lo + 1, (lo * 37) % (n - 1) + 0.5


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "bool"])
@pytest.mark.parametrize("n", [2, 257, 258])
def test_path_forest_comes_out_as_its_triples_in_order(ctx, n, valued):
    lo, hi, w = weighted_path(n)
    rows, cols, bits = sym(lo, hi, bits_of(w) if valued else None)
    W = upload(ctx, n, rows, cols, bits)
    comp, fr, fc, fw, st = engine.msf(ctx, W, stats=True)
    assert st[1] == len(fr) == len(fc) == len(fw) == n - 1
    assert np.array_equal(fr, lo.astype(U64)) and np.array_equal(fc, hi.astype(U64))   # (row, col) order, first and last row
    assert np.array_equal(fw.view(U64), bits_of(w if valued else np.ones(n - 1)))
    wc, _ = engine.wcc(ctx, W, None)
    assert np.array_equal(comp, wc) and np.all(comp == 0)


@pytest.mark.parametrize("n", [2, 257, 258])
def test_path_with_two_active_vertices_is_one_triple_or_none(ctx, n):
    lo, hi, w = weighted_path(n)
    rows, cols, bits = sym(lo, hi, bits_of(w))
    W = upload(ctx, n, rows, cols, bits)
    pairs = [(n - 2, n - 1)] + ([(0, n - 1)] if n > 2 else [])   # neighbours: their edge; the two ends: nothing
    for a, b in pairs:
        active = np.zeros(n, dtype=bool)
        active[[a, b]] = True
        comp, fr, fc, fw, st = engine.msf(ctx, W, bitmap(active), stats=True)
        want = np.full(n, -1, dtype=np.int64)
        if b == a + 1:
            want[[a, b]] = a
            assert fr.tolist() == [a] and fc.tolist() == [b] and np.array_equal(fw.view(U64), bits_of(w[a:a + 1]))
        else:
            want[a], want[b] = a, b
            assert len(fr) == len(fc) == len(fw) == 0
        assert np.array_equal(comp, want) and st[1] == len(fr)


def acyclic(n, fr, fc):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(fr.tolist(), fc.tolist()):
        a, b = find(a), find(b)
        if a == b:
            return False
        parent[max(a, b)] = min(a, b)
    return True


@pytest.mark.parametrize("one_direction", [False, True], ids=["asymmetric-values", "one-direction-stored"])
def test_broken_symmetry_promise_still_returns_a_forest(ctx, one_direction):
    rng = np.random.default_rng(17)
    n, m = 400, 1500
    lo, hi = random_pairs(rng, n, m)
    if one_direction:
        flip = rng.random(m) < 0.5
        rows, cols = np.where(flip, hi, lo), np.where(flip, lo, hi)
        bits = bits_of(rng.integers(0, 50, m).astype(np.float64))
    else:
        rows, cols = np.concatenate([lo, hi]), np.concatenate([hi, lo])
        bits = bits_of(rng.integers(0, 50, 2 * m).astype(np.float64))
    W = upload(ctx, n, rows, cols, bits)
    comp, fr, fc, fw, st = engine.msf(ctx, W, stats=True)
    assert len(fr) == st[1] == n - components(comp) and st[3] == components(comp)
    assert np.all(fr < fc) and acyclic(n, fr, fc)
    assert np.array_equal(comp[fr.astype(np.int64)], comp[fc.astype(np.int64)])
    assert np.all(comp[comp] == comp) and np.all(comp <= np.arange(n))


def test_error_codes(ctx):
    import ctypes as C
    lib = ctx.lib
    W = ctx.mat_new(4, 4)
    r, c, w = _ffi.u64p(), _ffi.u64p(), C.POINTER(C.c_double)()
    k = C.c_uint64(7)
    args = [C.byref(r), C.byref(c), C.byref(w), C.byref(k)]
    assert lib.fgpu_msf(None, W._h, None, None, *args, None) == _ffi.FGPU_NULL_POINTER
    assert lib.fgpu_msf(ctx._h, None, None, None, *args, None) == _ffi.FGPU_NULL_POINTER
    for i in range(4):
        bad = list(args)
        bad[i] = None
        assert lib.fgpu_msf(ctx._h, W._h, None, None, *bad, None) == _ffi.FGPU_NULL_POINTER
    with pytest.raises(FgpuError) as e:
        engine.msf(ctx, ctx.mat_new(3, 4))
    assert e.value.code == _ffi.FGPU_DIM_MISMATCH
    # nrows >= 2^32 - 1 is FGPU_INVALID in fgpu_msf (check_adjacency), but no constructor hands out such a snapshot: they refuse
    # the dimensions with the same code
    with pytest.raises(FgpuError) as e:
        ctx.mat_new(2**32 - 1, 2**32 - 1)
    assert e.value.code == _ffi.FGPU_INVALID
    assert lib.fgpu_msf(ctx._h, ctx.mat_new(0, 0)._h, None, None, *args, None) == _ffi.FGPU_OK and k.value == 0
    assert lib.fgpu_msf(ctx._h, W._h, None, None, *args, None) == _ffi.FGPU_OK and k.value == 0   # component is nullable
