"""fgpu_edges_build (csrc/edges.hip): one relationship type's bulk batch -> forward matrix with inline ids / MULTI_EDGE, the
transposed pattern and the ascending id runs of the multi-edge pairs.  The checker is a plain dict, pairs[(s, d)] -> sorted ids;
the pattern is also held to fgpu_mat_from_coo of the same pairs and its transpose."""
import ctypes as C

import numpy as np
import pytest

from falkordb_amd import _ffi, engine

pytestmark = pytest.mark.gpu

MULTI = 2**64 - 1


def model(srcs, dsts, ids):
    pairs = {}
    for s, d, i in zip(map(int, srcs), map(int, dsts), map(int, ids)):
        pairs.setdefault((s, d), []).append(i)
    for v in pairs.values():
        v.sort()
    return pairs


def check_build(ctx, nrows, ncols, srcs, dsts, ids):
    """Build, compare everything with the model, return the stats."""
    srcs, dsts, ids = (np.asarray(a, dtype=np.uint64) for a in (srcs, dsts, ids))
    fwd, bwd, mkey, moff, mids, st = engine.edges_build(ctx, nrows, ncols, srcs, dsts, ids, stats=True)
    pairs = model(srcs, dsts, ids)
    order = sorted(pairs)
    assert (fwd.nrows, fwd.ncols, bwd.nrows, bwd.ncols) == (nrows, ncols, ncols, nrows)
    # forward matrix: one entry per distinct pair, the id inline or the marker
    rp, ci, vals = fwd.export_csr()
    want_rp = np.zeros(nrows + 1, dtype=np.uint64)
    for s, _ in order:
        want_rp[s + 1] += 1
    want_rp = np.cumsum(want_rp).astype(np.uint64)
    assert np.array_equal(rp, want_rp)
    assert ci.tolist() == [d for _, d in order]
    assert vals is not None and vals.tolist() == [pairs[p][0] if len(pairs[p]) == 1 else MULTI for p in order]
    # ... its pattern = the COO builder's, bwd = that pattern transposed
    pat = ctx.mat_from_coo(nrows, ncols, srcs, dsts)
    prp, pci, _ = pat.export_csr()
    assert np.array_equal(rp, prp) and np.array_equal(ci, pci)
    trp, tci, _ = pat.transpose().export_csr()
    brp, bci, bvals = bwd.export_csr()
    assert bvals is None
    assert np.array_equal(brp, trp) and np.array_equal(bci, tci)
    # multi-edge rows
    multi = [p for p in order if len(pairs[p]) > 1]
    assert mkey.tolist() == [(s << 32) | d for s, d in multi]
    assert len(moff) == len(multi) + 1 and int(moff[0]) == 0
    assert np.diff(moff.astype(np.int64)).tolist() == [len(pairs[p]) for p in multi]
    assert mids.tolist() == [i for p in multi for i in pairs[p]]
    # counters
    assert st[0] == len(order) and st[1] == len(multi) and st[2] == len(mids)
    assert st[3] == max((len(v) for v in pairs.values()), default=0)
    assert st[4] == st[5] + st[6]
    assert st[7] == (0 if len(srcs) < 4096 else 1)
    return st


def test_empty_and_single(ctx):
    st = check_build(ctx, 5, 7, [], [], [])
    assert st[:7] == [0] * 7
    st = check_build(ctx, 5, 7, [4], [6], [123456789012345])
    assert st[:5] == [1, 0, 0, 1, 0]


@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
def test_wave_boundaries(ctx, n, shuffled):
    """64 x 64, tuples from 16 distinct pairs only: runs cross wavefront boundaries of the lane-per-position pass, and the
    shuffled ids put every run through the wavefront sort."""
    rng = np.random.default_rng(100 + n)
    ps, pd = rng.integers(0, 64, 16), rng.integers(0, 64, 16)
    pick = rng.integers(0, 16, n)
    ids = rng.permutation(n) if shuffled else np.arange(n)
    st = check_build(ctx, 64, 64, ps[pick], pd[pick], ids + 1000)
    if not shuffled:
        assert st[4] == 0
    assert st[6] == 0


@pytest.mark.parametrize("n", [257, 300, 4096, 4097, 5000])
def test_long_run_on_one_pair(ctx, n):
    """One pair, n parallel edges (+ one single-edge pair before and after it): ascending ids sort nothing; shuffled ids come
    out ascending, on the device up to 4096 ids and by the host past that."""
    s = np.concatenate([[1], np.full(n, 3), [6]])
    d = np.concatenate([[2], np.full(n, 5), [0]])
    asc = np.arange(n + 2) + 7
    st = check_build(ctx, 8, 8, s, d, asc)
    assert st[3] == n and st[4] == 0 and st[6] == 0
    ids = asc.copy()
    ids[1:n + 1] = np.random.default_rng(n).permutation(ids[1:n + 1])
    st = check_build(ctx, 8, 8, s, d, ids)
    assert st[4] == 1
    if n > 4096:
        assert st[6] >= 1
    else:
        assert st[6] == 0 and st[5] == 1


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_sort_path_thresholds(ctx, n):
    rng = np.random.default_rng(n)
    s, d = rng.integers(0, 4096, n), rng.integers(0, 4096, n)
    s[n // 2:] = s[:n - n // 2]   # half the tuples repeat a pair of the other half, in another position
    d[n // 2:] = d[:n - n // 2]
    st = check_build(ctx, 4096, 4096, s, d, rng.permutation(n))
    assert st[7] == (0 if n < 4096 else 1)
    assert st[1] > 0


def test_large_skewed_batch(ctx):
    """200 000 tuples on 2^16 vertices, about one in five a repeat of an earlier pair, ids shuffled and offset by 2^40."""
    rng = np.random.default_rng(20000)
    n, fresh = 200000, 160000
    hub = (rng.random(fresh) < 0.2)
    s = np.where(hub, rng.integers(0, 16, fresh), rng.integers(0, 65536, fresh))
    d = rng.integers(0, 65536, fresh)
    again = rng.integers(0, fresh, n - fresh)
    s, d = np.concatenate([s, s[again]]), np.concatenate([d, d[again]])
    mix = rng.permutation(n)
    st = check_build(ctx, 65536, 65536, s[mix], d[mix], rng.permutation(n).astype(np.uint64) + (1 << 40))
    assert st[1] > 10000 and st[4] > 0 and st[6] == 0


@pytest.mark.parametrize("n", [500, 6000])
def test_rectangular(ctx, n):
    rng = np.random.default_rng(n)
    st = check_build(ctx, 100, 3000, rng.integers(0, 100, n), rng.integers(0, 3000, n // 50, dtype=np.int64).repeat(50)[:n],
                     rng.permutation(n))
    assert st[1] > 0


@pytest.mark.parametrize("n", [8, 5000])
def test_edges_of_the_index_space(ctx, n):
    """Entries in row 0 / row nrows - 1 and column 0 / ncols - 1 only; then the same shape moved inside, so that leading and
    trailing rows are empty; then a row space wide enough for the staged levels of the counting sort."""
    rng = np.random.default_rng(n)
    for nrows, ncols, rows, cols in ((1000, 777, (0, 999), (0, 776)), (1000, 777, (400, 401), (0, 776)),
                                     ((1 << 17) + 3, 5, (0, (1 << 17) + 2), (0, 4)), (1, 1, (0, 0), (0, 0))):
        s = np.asarray(rows)[rng.integers(0, 2, n)]
        d = np.asarray(cols)[rng.integers(0, 2, n)]
        check_build(ctx, nrows, ncols, s, d, np.arange(n))


def test_a_dimension_past_2_31_sorts_in_16_bit_digits(ctx):
    """The counting sort takes key spaces up to 2^31; a wider row space goes through 16-bit digit passes, and that route exists at
    this size only.  The forward matrix is read a row at a time (its whole row pointer array would be 16 GiB on the host)."""
    nrows, ncols, n = 2**31 + 5, 7, 5000
    rows = np.array([0, 65535, 65536, 2**31 - 1, 2**31, 2**31 + 4], dtype=np.uint64)
    rng = np.random.default_rng(31)
    s, d, ids = rows[rng.integers(0, len(rows), n)], rng.integers(0, ncols, n).astype(np.uint64), rng.permutation(n)
    fwd, bwd, mkey, moff, mids, st = engine.edges_build(ctx, nrows, ncols, s, d, ids, stats=True)
    pairs = model(s, d, ids)
    order = sorted(pairs)
    multi = [p for p in order if len(pairs[p]) > 1]
    assert st[7] == 2 and st[0] == len(order) == fwd.nvals and st[1] == len(multi)
    got = []
    for r in rows.tolist():
        rr, cc, vv = fwd.extract(r, r)
        got += list(zip(rr.tolist(), cc.tolist(), vv.tolist()))
    assert got == [(p[0], p[1], pairs[p][0] if len(pairs[p]) == 1 else MULTI) for p in order]
    for r in (1, 65537, 2**31 - 2, 2**31 + 1, 2**31 + 3):       # the rows between them are empty
        assert len(fwd.extract(r, r)[0]) == 0
    brp, bci, _ = bwd.export_csr()
    back = sorted((dd, ss) for ss, dd in order)
    assert bci.tolist() == [ss for _, ss in back]
    assert np.diff(brp.astype(np.int64)).tolist() == [sum(1 for dd, _ in back if dd == c) for c in range(ncols)]
    assert mkey.tolist() == [(a << 32) | b for a, b in multi]
    assert np.diff(moff.astype(np.int64)).tolist() == [len(pairs[p]) for p in multi]
    assert mids.tolist() == [i for p in multi for i in pairs[p]]


def _raises_invalid(fn):
    with pytest.raises(_ffi.FgpuError) as e:
        fn()
    assert e.value.code == _ffi.FGPU_INVALID
    assert str(e.value).split(":", 1)[1].strip()   # fgpu_last_error is set


def test_rejections_leave_the_context_usable(ctx):
    good = ([0, 1, 1, 2], [1, 2, 2, 0], [10, 12, 11, 13])
    big = np.arange(5000)
    cases = [
        lambda: engine.edges_build(ctx, 3, 3, [3], [0], [1]),                      # source at its dimension
        lambda: engine.edges_build(ctx, 3, 3, [0], [7], [1]),                      # destination past its dimension
        lambda: engine.edges_build(ctx, 2**32 - 1, 3, [0], [0], [1]),              # dimension past the 32-bit id space
        lambda: engine.edges_build(ctx, 3, 2**32, [0], [0], [1]),
        lambda: engine.edges_build(ctx, 3, 3, [0, 1], [0, 1], [5, MULTI]),         # the marker as an id
        lambda: engine.edges_build(ctx, 3, 3, [1, 1], [2, 2], [9, 9]),             # the same triple twice, adjacent
        lambda: engine.edges_build(ctx, 3, 3, [1, 0, 1, 1], [2, 0, 2, 2], [9, 4, 11, 9]),   # ... apart: found after the wavefront sort
        lambda: engine.edges_build(ctx, 3, 3, np.ones(300), np.ones(300), np.r_[np.arange(299, 0, -1), 150]),   # workgroup sort
        lambda: engine.edges_build(ctx, 3, 3, big * 0 + 2, big * 0, np.r_[big[:0:-1], 2500]),                   # host sort
        lambda: engine.edges_build(ctx, 4096, 4096, np.r_[big, 77] % 4096, np.r_[big, 77] % 4096, np.r_[big, 77]),  # counting path
    ]
    for bad in cases:
        before = ctx.device_bytes()[0]
        _raises_invalid(bad)
        assert ctx.device_bytes()[0] == before, "a rejected batch keeps device memory"
        check_build(ctx, 3, 3, *good)                                              # the next call is exact


def test_too_many_tuples_is_rejected_before_the_arrays_are_read(ctx):
    """n >= 2^32 - 1: the count alone is refused (the arrays behind it are never touched, so one element stands in)."""
    one = np.zeros(1, dtype=np.uint64)
    p = one.ctypes.data_as(_ffi.u64p)
    fwd, bwd = C.c_void_p(), C.c_void_p()
    mk, mo, mi = _ffi.u64p(), _ffi.u64p(), _ffi.u64p()
    nm = C.c_uint64()
    for n in (2**32 - 1, 2**32):
        code = ctx.lib.fgpu_edges_build(ctx.handle, 3, 3, p, p, p, C.c_uint64(n), C.byref(fwd), C.byref(bwd), C.byref(mk),
                                        C.byref(mo), C.byref(mi), C.byref(nm), None)
        assert code == _ffi.FGPU_INVALID and ctx.lib.fgpu_last_error()
        assert not fwd.value and not bwd.value and not mk and not mo and not mi and nm.value == 0
    check_build(ctx, 3, 3, [0, 1, 1, 2], [1, 2, 2, 0], [10, 12, 11, 13])
