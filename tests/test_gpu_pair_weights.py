"""fgpu_pair_weights (csrc/pair_weights.hip): the algorithms' weighted pair matrix built on the device.  The expected value is
always tests/pair_weights_check.py over the effective relationships of the same layers, and every comparison is exact: W's bit
patterns, K's ids, the pattern and all eight stats.  Shapes are the smallest at which a pass can go wrong: entry counts around
one 64-entry word, hypersparse layers, id rows around one wavefront and past one workgroup, attribute lists around the binary
search's edges, one pair with more candidates than a workgroup holds, and one seeded multigraph of 2 000 nodes."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_weights_check as pw  # noqa: E402
from msf_check import ONE_BITS, bits_of, msf  # noqa: E402
from sssp_check import sssp  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64
MULTI = (1 << 64) - 1
INF, NAN = math.inf, math.nan


# ---- one tensor's layers, in Python and on the device --------------------------------------------------------------------
class Ten:
    """m / dp: {(src, dst): inline id or MULTI}; dm: a set of pairs; me: {(src, dst): ascending ids} for the MULTI pairs"""

    def __init__(self, name, m=None, dp=None, dm=None, me=None):
        self.name, self.m, self.dp, self.dm, self.me = name, dict(m or {}), dict(dp or {}), set(dm or ()), dict(me or {})

    def effective(self):
        """Tensor::iter_edges: (type, src, dst, id) over (pattern(m) \\ dm) U pattern(dp), dp's value winning"""
        vals = {k: v for k, v in self.m.items() if k not in self.dm}
        vals.update(self.dp)
        return [(self.name, s, d, i) for (s, d), v in vals.items() for i in (self.me[(s, d)] if v == MULTI else [v])]


def _coo(ctx, n, entries, valued):
    keys = sorted(entries)
    if not keys:
        return None
    r = np.array([k[0] for k in keys], dtype=U64)
    c = np.array([k[1] for k in keys], dtype=U64)
    return ctx.mat_from_coo(n, n, r, c, np.array([entries[k] for k in keys], dtype=U64) if valued else None)


class Dev:
    def __init__(self, ctx, n, t, null_deltas=False):
        self.m = _coo(ctx, n, t.m, True) or ctx.mat_new(n, n)
        self.dp = _coo(ctx, n, t.dp, True)
        self.dm = _coo(ctx, n, {k: 1 for k in t.dm}, False)
        if not null_deltas:   # an empty layer as a handle, not as NULL
            self.dp = self.dp or ctx.mat_new(n, n)
            self.dm = self.dm or ctx.mat_new(n, n)
        keys = sorted(t.me)
        self.multi = None
        if keys:
            off = np.concatenate([[0], np.cumsum([len(t.me[k]) for k in keys])]).astype(U64)
            self.multi = ctx.multi_new(np.array([(s << 32) | d for s, d in keys], dtype=U64), off,
                                       np.array([x for k in keys for x in t.me[k]], dtype=U64))


def bitmap(active):
    words = np.zeros((len(active) + 63) // 64, dtype=U64)
    for v in np.flatnonzero(active):
        words[v >> 6] |= U64(1) << U64(v & 63)
    return words


def call(ctx, devs, flags, attr=None, missing=1.0, active=None, **kw):
    ids = vals = None
    if attr is not None:
        ids = np.array(sorted(attr), dtype=U64)
        vals = np.array([attr[i] for i in sorted(attr)], dtype=np.float64)
    return ctx.pair_weights([d.m for d in devs], [d.dp for d in devs], [d.dm for d in devs], [d.multi for d in devs],
                            out=bool(flags & pw.OUT), inc=bool(flags & pw.IN), negate=bool(flags & pw.NEGATE),
                            drop_nonfinite=bool(flags & pw.DROP_NONFINITE), refuse_negative=bool(flags & pw.REFUSE_NEGATIVE),
                            active_bitmap=None if active is None else bitmap(active), attr_ids=ids, attr_vals=vals,
                            missing=missing, **kw)


def same(W, K, st, want):
    rows, cols, bits, kept, wst = want
    wr, wc, wv = W.extract()
    kr, kc, kv = K.extract()
    assert np.array_equal(wr, rows) and np.array_equal(wc, cols) and np.array_equal(kr, rows) and np.array_equal(kc, cols)
    assert W.has_values == (bits is not None) and K.has_values
    if len(rows):
        assert bits is None or np.array_equal(wv, bits)
        assert np.array_equal(kv, kept)
    assert st == wst, (st, wst)


def check(ctx, n, tens, flags, attr=None, missing=1.0, active=None, devs=None):
    devs = devs or [Dev(ctx, n, t) for t in tens]
    W, K, st = call(ctx, devs, flags, attr, missing, active)
    want = pw.pair_weights(n, [r for t in tens for r in t.effective()], attr, flags, active, missing)
    same(W, K, st, want)
    return want


def invalid(ctx, devs, flags, attr_ids=None, attr_vals=None, **kw):
    with pytest.raises(_ffi.FgpuError) as e:
        ctx.pair_weights([d.m for d in devs], [d.dp for d in devs], [d.dm for d in devs], [d.multi for d in devs],
                         out=bool(flags & pw.OUT), inc=bool(flags & pw.IN), attr_ids=attr_ids, attr_vals=attr_vals, **kw)
    assert e.value.code == _ffi.FGPU_INVALID
    return e.value


BOTH = pw.OUT | pw.IN
SP = pw.DROP_NONFINITE | pw.REFUSE_NEGATIVE


def scattered(count, n, seed=1):
    """`count` distinct pairs in a handful of rows (hypersparse past 4096 rows), no self-loop"""
    rng = np.random.default_rng(seed)
    pairs = {}
    rows = [1, 63, 64, n - 1, n // 2]
    while len(pairs) < count:
        s, d = rows[int(rng.integers(0, len(rows)))], int(rng.integers(0, n))
        if s != d:
            pairs[(s, d)] = 1000 + len(pairs)
    return pairs


# ---- one type, clean base -----------------------------------------------------------------------------------------------
def test_one_clean_type_with_unit_weights_gives_a_bool_w_and_the_inline_ids(ctx):
    n = 300
    m = {(v, (v * 7 + 3) % n): 5000 + v for v in range(n) if (v * 7 + 3) % n != v}
    t = Ten("A", m)
    d = Dev(ctx, n, t, null_deltas=True)
    W, K, st = call(ctx, [d], pw.OUT)
    assert not W.has_values and K.has_values
    r, c, v = K.extract()
    assert {(int(a), int(b)): int(x) for a, b, x in zip(r, c, v)} == m
    wr, wc, _ = W.extract()
    assert np.array_equal(wr, r) and np.array_equal(wc, c)
    assert st == [len(m), len(m), len(m), len(m), 0, 0, 0, 1]
    check(ctx, n, [t], pw.OUT, devs=[d])


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 129])
def test_entry_counts_around_the_word_edge(ctx, count):
    n = 5003                                   # not a multiple of 64; five populated rows: the layers are hypersparse
    t = Ten("A", scattered(count, n))
    attr = {1000 + k: float(k % 7) for k in range(0, count, 2)}
    want = check(ctx, n, [t], BOTH, attr, INF)
    assert want[4][0] == count
    check(ctx, n, [t], pw.IN)
    half = scattered(count, n, seed=2)         # the same count split over m and dp
    keys = sorted(half)
    t2 = Ten("A", {k: half[k] for k in keys[::2]}, dp={k: half[k] for k in keys[1::2]})
    check(ctx, n, [t2], pw.OUT, attr, 1.0)


def test_nothing_examined_gives_empty_matrices(ctx):
    n = 70
    t = Ten("A", {(3, 3): 1, (4, 5): 2}, dm={(4, 5)})
    W, K, st = call(ctx, [Dev(ctx, n, t)], BOTH, {1: 1.0})
    assert (W.nrows, W.ncols, W.nvals, K.nrows, K.nvals) == (n, n, 0, n, 0) and W.has_values and K.has_values
    assert st == [0] * 8
    W, K, st = call(ctx, [Dev(ctx, n, Ten("A"))], pw.OUT)
    assert W.nvals == 0 and not W.has_values and K.nvals == 0


# ---- Delta layers -------------------------------------------------------------------------------------------------------
def test_delta_layers(ctx):
    n = 130
    a = Ten("A", m={(1, 2): 10, (1, 3): 11, (64, 65): 12, (5, 6): MULTI, (7, 8): 13},
            dp={(1, 2): 20,               # overrides m's value on the same pair
                (9, 10): 21,              # a dp-only pair
                (5, 6): 22,               # a single id over a multi-edge pair of m
                (7, 8): MULTI},           # a multi-edge over a single id of m
            dm={(1, 3), (5, 6)},          # hides m's (1, 3); (5, 6) is dp's anyway
            me={(7, 8): [13, 23, 24]})
    b = Ten("B", m={(1, 2): 30, (1, 3): 31, (129, 0): 32})
    attr = {10: 0.5, 20: 4.0, 30: 5.0, 11: 0.1, 31: 6.0, 13: 3.0, 23: 2.0, 24: 2.5, 22: 1.5}
    devs = [Dev(ctx, n, a), Dev(ctx, n, b, null_deltas=True)]   # B's dp / dm are NULL beside A's
    for flags in (pw.OUT, pw.IN, BOTH):
        rows, cols, bits, kept, st = check(ctx, n, [a, b], flags, attr, 9.0, devs=devs)
    got = {(int(r), int(c)): (float(x), int(k)) for r, c, x, k in zip(rows, cols, bits.view(np.float64), kept)}
    assert got[(1, 2)] == (4.0, 20) and got[(1, 3)] == (6.0, 31) and got[(5, 6)] == (1.5, 22) and got[(7, 8)] == (2.0, 23)
    assert got[(9, 10)] == (9.0, 21) and got[(10, 9)] == (9.0, 21)
    check(ctx, n, [a, b], pw.OUT, devs=devs)


# ---- multi-edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "middle", "tie"])
def test_multi_edge_rows(ctx, where):
    n = 200
    lens = [2, 64, 65, 200]
    m, me, attr = {(0, 9): 7}, {}, {7: 1.0}
    base = 100
    for k, ln in enumerate(lens):
        pair = (10 + k, 20 + k)
        ids = list(range(base, base + 3 * ln, 3))
        base += 3 * ln + 5
        m[pair], me[pair] = MULTI, ids
        for j, i in enumerate(ids):
            attr[i] = 10.0 + (j * 37) % 11
        low = {"first": [ids[0]], "last": [ids[-1]], "middle": [ids[ln // 2]], "tie": [ids[-1], ids[ln // 2]]}[where]
        for i in low:
            attr[i] = 0.25
    t = Ten("A", m, me=me)
    rows, cols, bits, kept, st = check(ctx, n, [t], pw.OUT, attr)
    assert st[6] == 4 and st[7] == 200 and st[1] == 1 + sum(lens)
    for k, ln in enumerate(lens):
        ids = me[(10 + k, 20 + k)]
        want = {"first": ids[0], "last": ids[-1], "middle": ids[ln // 2], "tie": ids[ln // 2]}[where]
        assert int(kept[list(rows).index(10 + k)]) == want
    check(ctx, n, [t], BOTH)   # unit weights: the smallest id of every row


def test_a_multi_edge_pair_without_a_table_row_is_invalid_and_the_context_survives(ctx):
    n = 80
    t = Ten("A", {(1, 2): MULTI, (3, 4): MULTI, (5, 6): 9}, me={(1, 2): [4, 5], (3, 4): [6, 7]})
    short = Ten("A", t.m, me={(1, 2): [4, 5]})
    d = Dev(ctx, n, short)
    e = invalid(ctx, [d], pw.OUT)
    assert "no row" in str(e)
    d.multi = None
    invalid(ctx, [d], BOTH, np.array([4], dtype=U64), np.array([1.0]))
    hidden = Ten("A", t.m, me={(1, 2): [4, 5]}, dm={(3, 4)})   # the pair without a row is not visited: fine
    check(ctx, n, [hidden], pw.OUT)
    check(ctx, n, [t], pw.OUT)


# ---- several types ------------------------------------------------------------------------------------------------------
def test_the_same_pair_in_three_types_and_a_type_listed_twice(ctx):
    n = 66
    tens = [Ten("A", {(1, 2): 30, (2, 1): 3}), Ten("B", {(1, 2): 10, (65, 0): 4}), Ten("C", {(1, 2): 20})]
    attr = {30: 2.0, 10: 2.0, 20: 2.0, 3: 2.0, 4: 1.0}
    devs = [Dev(ctx, n, t) for t in tens]
    for order in itertools.permutations(range(3)):
        rows, cols, bits, kept, st = check(ctx, n, [tens[i] for i in order], pw.OUT, attr, devs=[devs[i] for i in order])
        assert int(kept[0]) == 10 and st[7] == 3
    rows, cols, bits, kept, st = check(ctx, n, tens, BOTH, attr, devs=devs)
    assert kept.tolist() == [4, 3, 3, 4]
    once = call(ctx, devs, BOTH, attr)
    twice = call(ctx, devs + [devs[1], devs[0]], BOTH, attr)
    assert twice[2] == once[2]
    same(twice[0], twice[1], twice[2], (rows, cols, bits, kept, st))


def test_sixty_four_types_and_one_more(ctx):
    n = 100
    tens = [Ten(f"T{k}", {(k, (k * 3 + 1) % n): 500 - k} if k % 5 else {(1, 4): 500 - k}) for k in range(65)]
    devs = [Dev(ctx, n, t, null_deltas=True) for t in tens]
    attr = {500 - k: float(k % 3) for k in range(65)}
    check(ctx, n, tens[:64], BOTH, attr, devs=devs[:64])
    invalid(ctx, devs, pw.OUT)
    with pytest.raises(_ffi.FgpuError) as e:
        ctx.pair_weights([], [], [], [])
    assert e.value.code == _ffi.FGPU_INVALID


# ---- direction, self-loops, the active set ------------------------------------------------------------------------------
def test_direction_self_loops_and_the_active_set(ctx):
    n = 70
    t = Ten("A", {(1, 2): 1, (2, 1): 2, (3, 3): 3, (4, 5): 4, (64, 69): 5, (69, 4): 6, (6, 6): MULTI}, me={(6, 6): [7, 8]})
    attr = {1: 5.0, 2: 3.0, 3: 0.5, 4: 1.0, 5: 2.0, 6: 4.0, 7: 1.0, 8: 1.0}
    d = [Dev(ctx, n, t)]
    out = check(ctx, n, [t], pw.OUT, attr, devs=d)
    inc = check(ctx, n, [t], pw.IN, attr, devs=d)
    both = check(ctx, n, [t], BOTH, attr, devs=d)
    assert sorted(zip(out[0].tolist(), out[1].tolist())) == sorted(zip(inc[1].tolist(), inc[0].tolist()))
    got = {(int(r), int(c)): (float(x), int(k)) for r, c, x, k in zip(both[0], both[1], both[2].view(np.float64), both[3])}
    assert got[(1, 2)] == got[(2, 1)] == (3.0, 2)                      # both ordered pairs carry the smaller
    assert all(got[(c, r)] == v for (r, c), v in got.items())          # W and K are symmetric
    assert all(r != c for r, c in got) and both[4][1] == 5             # the self-loops (one a multi-edge) are not examined
    one_end = np.ones(n, dtype=bool)
    one_end[69] = False
    want = check(ctx, n, [t], BOTH, attr, active=one_end, devs=d)
    assert want[4][1] == 3
    both_ends = one_end.copy()
    both_ends[64] = False
    assert check(ctx, n, [t], BOTH, attr, active=both_ends, devs=d)[4][1] == 3
    none = np.zeros(n, dtype=bool)
    assert check(ctx, n, [t], BOTH, attr, active=none, devs=d)[4] == [0] * 8


# ---- attributes ---------------------------------------------------------------------------------------------------------
def chain(n_rel, first_id=100, step=1):
    return Ten("A", {(k, k + 1): first_id + k * step for k in range(n_rel)})


@pytest.mark.parametrize("missing", [INF, 1.0])
def test_ids_below_above_and_between_the_listed_ones_take_missing(ctx, missing):
    n = 40
    t = chain(30)                                                  # ids 100 .. 129
    attr = {i: 0.5 * (i - 100) for i in list(range(105, 110)) + list(range(115, 120))}   # below, a gap, above
    for flags in (pw.OUT, BOTH | pw.NEGATE, pw.OUT | pw.DROP_NONFINITE):
        want = check(ctx, n, [t], flags, attr, missing)
        assert want[4][5] == 20
    neg = check(ctx, n, [t], pw.OUT | pw.NEGATE, attr, missing)    # NEGATE on the listed values only
    w = neg[2].view(np.float64)
    assert w[5] == -2.5 and w[0] == missing and w[29] == missing


def test_zero_signs_and_non_finite_weights(ctx):
    n = 20
    t = Ten("A", {(0, 1): 1, (1, 2): 2, (2, 3): 3, (3, 4): 4, (4, 5): 5, (5, 6): MULTI, (7, 8): MULTI},
            me={(5, 6): [6, 7, 8], (7, 8): [9, 10]})
    attr = {1: -0.0, 2: 0.0, 3: NAN, 4: INF, 5: -INF, 6: NAN, 7: INF, 8: 2.0, 9: NAN, 10: -NAN}
    rows, cols, bits, kept, st = check(ctx, n, [t], pw.OUT, attr)
    assert bits[0] == 0 and bits[1] == 0 and kept.tolist() == [1, 2, 3, 4, 5, 8, 10]   # the NaNs order by their bits
    rows, cols, bits, kept, st = check(ctx, n, [t], pw.OUT | pw.NEGATE, attr)
    assert bits[0] == 0 and bits[1] == 0                                             # 0.0 under NEGATE comes out as +0.0
    rows, cols, bits, kept, st = check(ctx, n, [t], BOTH | pw.DROP_NONFINITE, attr)
    assert st[4] == 7 and kept.tolist() == [1, 1, 2, 2, 8, 8]
    check(ctx, n, [t], pw.OUT | SP, attr)                                             # -inf and -NaN are dropped, not refused
    check(ctx, n, [t], pw.OUT | pw.REFUSE_NEGATIVE, attr)                             # ... and not refused when kept either
    check(ctx, n, [t], pw.IN | pw.DROP_NONFINITE, {}, NAN)                            # a list of nothing: all take `missing`


@pytest.mark.parametrize("n_attr", [1, 64, 65])
def test_attribute_lists_around_the_binary_search_edges(ctx, n_attr):
    n = 140
    t = chain(135, first_id=10, step=2)                            # ids 10, 12, .. 278
    for first in (10, 9, 150):                                     # hits from the first id, only misses below, the upper half
        attr = {first + 2 * k: float((k * 5) % 9) for k in range(n_attr)}
        check(ctx, n, [t], pw.OUT, attr, 7.5)


def test_attr_ids_must_ascend_strictly(ctx):
    n = 10
    d = [Dev(ctx, n, chain(5))]
    vals = np.arange(70, dtype=np.float64)
    ids = np.arange(100, 170, dtype=U64)
    for k in (0, 33, 68):
        eq = ids.copy()
        eq[k + 1] = eq[k]
        assert "ascending" in str(invalid(ctx, d, pw.OUT, eq, vals))
        desc = ids.copy()
        desc[k], desc[k + 1] = desc[k + 1], desc[k]
        invalid(ctx, d, BOTH, desc, vals)
    W, K, st = ctx.pair_weights([d[0].m], out=True, attr_ids=ids, attr_vals=vals)
    assert st[3] == 5
    invalid(ctx, [Dev(ctx, n, Ten("A"))], pw.OUT, ids[::-1].copy(), vals)   # checked even when nothing is examined


def test_flags_are_checked(ctx):
    d = [Dev(ctx, 10, chain(5))]
    invalid(ctx, d, 0)
    code = ctx.lib.fgpu_pair_weights(ctx._h, engine._hop_arrays([d[0].m]), None, None, None, 1, 33, None, None, None, 0, 1.0, None,
                                     None, None, None)
    assert code == _ffi.FGPU_INVALID and b"unknown flag" in ctx.lib.fgpu_last_error()


# ---- refusal ------------------------------------------------------------------------------------------------------------
def test_refusal(ctx):
    n = 70
    t = Ten("A", {(1, 2): 40, (2, 3): 30, (3, 3): 5, (4, 69): 6, (5, 6): MULTI, (8, 9): 50}, me={(5, 6): [20, 35]})
    attr = {40: -1.0, 30: 1.0, 5: -9.0, 6: -9.0, 20: 2.0, 35: -0.5, 50: -0.0}
    d = [Dev(ctx, n, t)]
    active = np.ones(n, dtype=bool)
    active[69] = False
    with pytest.raises(pw.Refused) as want:
        pw.pair_weights(n, t.effective(), attr, pw.OUT | SP, active)
    assert want.value.id == 35
    with pytest.raises(_ffi.FgpuError) as e:
        call(ctx, d, pw.OUT | SP, attr, active=active)
    assert e.value.code == _ffi.FGPU_INVALID and e.value.refused_id == 35
    assert str(e.value).endswith("fgpu_pair_weights: relationship 35 has a negative weight")
    # the self-loop's and the deselected end's negative weights are not refused
    ok = dict(attr)
    ok[40], ok[35] = 1.0, 0.5
    check(ctx, n, [t], BOTH | SP, ok, active=active, devs=d)
    with pytest.raises(_ffi.FgpuError) as e:             # ... until the end is selected
        call(ctx, d, BOTH | SP, ok)
    assert e.value.refused_id == 6
    with pytest.raises(_ffi.FgpuError) as e:             # NEGATE turns the positive values negative
        call(ctx, d, pw.IN | pw.NEGATE | pw.REFUSE_NEGATIVE, ok, active=active)
    assert e.value.refused_id == 20
    # *W and *K are untouched after a refusal
    ids = np.array(sorted(attr), dtype=U64)
    vals = np.array([attr[i] for i in sorted(attr)], dtype=np.float64)
    w, k, refused = C.c_void_p(0x1234), C.c_void_p(0x5678), C.c_uint64(0)
    st = (C.c_uint64 * 8)()
    code = ctx.lib.fgpu_pair_weights(ctx._h, engine._hop_arrays([d[0].m]), engine._hop_arrays([d[0].dp]), engine._hop_arrays([d[0].dm]),
                                     engine._hop_arrays([d[0].multi]), 1, pw.OUT | SP, None, engine._p(ids),
                                     engine._p(vals, C.POINTER(C.c_double)), len(ids), 1.0, C.byref(w), C.byref(k), C.byref(refused), st)
    assert code == _ffi.FGPU_INVALID and (w.value, k.value, refused.value) == (0x1234, 0x5678, 6) and list(st) == [0] * 8


# ---- one pair with more candidates than a workgroup holds --------------------------------------------------------------
def test_a_hub_pair_past_one_workgroup(ctx):
    n = 64
    tens, attr = [], {}
    for k, name in enumerate("ABC"):
        ids = list(range(10_000 * (k + 1), 10_000 * (k + 1) + 700))
        m, me = {(7, 40): MULTI, (k, 50): 90 + k}, {(7, 40): ids}
        if k == 1:
            m[(40, 7)], me[(40, 7)] = MULTI, list(range(50_000, 50_700))
        tens.append(Ten(name, m, me=me))
        for j, i in enumerate(ids):
            attr[i] = 5.0 + ((j * 131 + k * 17) % 699)
    for i in range(50_000, 50_700):
        attr[i] = 6.0 + (i % 13)
    attr[20_345] = attr[30_699] = 5.0                       # the minimum three times: the smallest id wins
    rows, cols, bits, kept, st = check(ctx, n, tens, BOTH, attr, INF)
    assert st[7] == 2800 and st[6] == 4
    at = {(int(r), int(c)): int(k) for r, c, k in zip(rows, cols, kept)}
    assert at[(7, 40)] == at[(40, 7)] == 10_000
    assert check(ctx, n, tens, pw.OUT, attr)[4][7] == 2100
    assert check(ctx, n, tens, pw.IN)[4][7] == 2100


# ---- a seeded random multigraph ----------------------------------------------------------------------------------------
def random_tensors(seed, n=2000, n_rel=20_000):
    """3 types, about 5 % of the pairs multi-edge, a tenth of the relationships pending as additions and a twentieth as deletions"""
    rng = np.random.default_rng(seed)
    names = ["A", "B", "C"]
    committed, final = {}, {}
    for eid in range(n_rel):
        ty = names[int(rng.integers(0, 3))]
        s, d = (int(x) for x in rng.integers(0, n, 2))
        if rng.random() < 0.06 and final:                   # a parallel relationship, sometimes the other way round
            keys = list(final)
            ty, s, d = keys[int(rng.integers(0, len(keys)))]
            if rng.random() < 0.3:
                s, d = d, s
        pending = eid >= n_rel * 9 // 10
        final.setdefault((ty, s, d), []).append(eid)
        if not pending:
            committed.setdefault((ty, s, d), []).append(eid)
    for key in list(final):                                 # pending deletions of committed relationships
        keep = [i for i in final[key] if i >= n_rel * 9 // 10 or rng.random() >= 0.05]
        if keep:
            final[key] = keep
        else:
            del final[key]
    tens = {name: Ten(name) for name in names}
    for (ty, s, d), base in committed.items():
        t = tens[ty]
        t.m[(s, d)] = base[0] if len(base) == 1 else MULTI
        now = final.get((ty, s, d))
        if now is None:
            t.dm.add((s, d))
        elif now != base:
            t.dp[(s, d)] = now[0] if len(now) == 1 else MULTI
    for (ty, s, d), now in final.items():
        t = tens[ty]
        if (ty, s, d) not in committed:
            t.dp[(s, d)] = now[0] if len(now) == 1 else MULTI
        if len(now) >= 2:
            t.me[(s, d)] = now
    return n, [tens[x] for x in names], rng


@pytest.fixture(scope="module")
def random_graph(ctx):
    n, tens, rng = random_tensors(7)
    ids = sorted(i for t in tens for _, _, _, i in t.effective())
    pool = [0.0, -0.0, 0.25, 1.0, 1.0, 2.5, 7.0, 1e300, INF, NAN]
    attr = {i: pool[int(rng.integers(0, len(pool)))] for i in ids if rng.random() < 0.5}
    active = rng.random(n) < 0.9
    return n, tens, [Dev(ctx, n, t) for t in tens], attr, active


@pytest.mark.parametrize("direction", [pw.OUT, pw.IN, BOTH])
@pytest.mark.parametrize("flagset", ["msf", "sppaths"])
def test_seeded_random_multigraph(ctx, random_graph, direction, flagset):
    n, tens, devs, attr, active = random_graph
    if flagset == "msf":
        want = check(ctx, n, tens, direction | pw.NEGATE, attr, INF, active, devs=devs)
    else:
        want = check(ctx, n, tens, direction | SP, attr, 1.0, None, devs=devs)
        assert want[4][4] > 0
    assert want[4][6] > 300 and want[4][5] > 5000 and want[4][7] >= 2
    assert any(t.dp for t in tens) and any(t.dm for t in tens)


# ---- feeding the outputs on ---------------------------------------------------------------------------------------------
def test_the_outputs_feed_msf_and_sssp(ctx, random_graph):
    n, tens, devs, attr, active = random_graph
    finite = {i: (w if math.isfinite(w) else 3.0) for i, w in attr.items()}
    W, K, st = call(ctx, devs, BOTH, finite, INF, active)
    rows, cols, bits, kept, _ = pw.pair_weights(n, [r for t in tens for r in t.effective()], finite, BOTH, active, INF)
    comp, fr, fc, fw, _ = engine.msf(ctx, W, bitmap(active))
    wr, wc, wb, wcomp = msf(n, rows, cols, bits, active)
    assert np.array_equal(fr, wr) and np.array_equal(fc, wc) and np.array_equal(bits_of(fw), wb) and np.array_equal(comp, wcomp)
    present, ids = K.probe(fr, fc, want_vals=True)
    at = {(int(r), int(c)): int(k) for r, c, k in zip(rows, cols, kept)}
    assert present.all() and ids.tolist() == [at[(int(a), int(b))] for a, b in zip(fr, fc)]
    W, K, st = call(ctx, devs, pw.OUT | SP, attr, 1.0)
    rows, cols, bits, kept, _ = pw.pair_weights(n, [r for t in tens for r in t.effective()], attr, pw.OUT | SP, None, 1.0)
    for src in (0, 1234):
        dist, parent = engine.sssp(ctx, W, src)
        wd, wp, _ = sssp(n, rows, cols, bits, src)
        assert np.array_equal(dist.view(U64), wd.view(U64)) and np.array_equal(parent, wp)


def test_a_unit_bool_w_gives_the_forest_of_the_same_pattern_with_one_bits(ctx, random_graph):
    n, tens, devs, attr, active = random_graph
    W, K, st = call(ctx, devs, BOTH)
    assert not W.has_values
    r, c, _ = W.extract()
    ones = ctx.mat_from_coo(n, n, r, c, np.full(len(r), ONE_BITS, dtype=U64))
    a, b = engine.msf(ctx, W), engine.msf(ctx, ones)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and len(a[1]) > 0
    d0, p0 = engine.sssp(ctx, W, 5)
    d1, p1 = engine.sssp(ctx, ones, 5)
    assert np.array_equal(d0, d1) and np.array_equal(p0, p1)


def test_w_or_k_alone(ctx, random_graph):
    n, tens, devs, attr, active = random_graph
    W, K, st = call(ctx, devs, BOTH | pw.NEGATE, attr, INF, active)
    W1, none, st1 = call(ctx, devs, BOTH | pw.NEGATE, attr, INF, active, want_k=False)
    none2, K2, st2 = call(ctx, devs, BOTH | pw.NEGATE, attr, INF, active, want_w=False)
    assert none is None and none2 is None and st1 == st and st2 == st
    for a, b in ((W, W1), (K, K2)):
        assert all(np.array_equal(x, y) for x, y in zip(a.extract(), b.extract()))
    unit_k = call(ctx, devs, pw.OUT, want_w=False)[1]
    assert unit_k.has_values and unit_k.nvals == call(ctx, devs, pw.OUT, want_k=False)[0].nvals
