"""The case builders of tests/matrix_edges.py hold what their names claim, and their numpy references agree with the C oracle
(no GPU needed).  Every length and unique count is recomputed here from the inputs with Python sets."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402


def same(ref: me.Csr, orc: oracle.CSR):
    assert (ref.nrows, ref.ncols, ref.nnz) == (orc.nrows, orc.ncols, orc.nnz)
    np.testing.assert_array_equal(ref.rowptr, orc.rowptr)
    np.testing.assert_array_equal(ref.colidx, orc.colidx)


def orc(a: me.Csr) -> oracle.CSR:
    return oracle.CSR(a.nrows, a.ncols, a.rowptr, a.colidx)


@pytest.mark.parametrize("N", me.WIDE_KEY_SPACES)
def test_wide_sort_cases_reach_the_largest_legal_id(N):
    """Past 2^31 the numpy references stand alone (the oracle's product allocates per column): every claim below holds for
    them too, keys with bit 31 set are in every class, and N - 1 — one below the sorts' padding value at 2^32 - 2 — is stored."""
    assert (1 << 31) < N <= (1 << 32) - 2
    sc = me.sort_cases(N)
    assert int(sc.B.colidx.max()) == N - 1 == int(sc.C.colidx.max()) and int(sc.B.colidx.min()) == 0
    for i, (name, L, uniq) in sc.claims.items():
        if name.endswith(("-ends", "-below")):
            assert int(sc.C.row(i).max()) == N - 1 and int(sc.C.row(i).min()) == 0, name
            assert len(sc.C.row(i)) == uniq == L, name
    assert sc.dup_key == N // 3
    r, c = sc.coo()
    assert len(r) >= 4096 and int(c.max()) == N - 1
    assert me.build(sc.F.nrows, N, r, c).to_set() == sc.C.to_set()
    m, dp, dm = sc.layers()
    assert me.merge(m, dp, None).to_set() == sc.C.to_set()
    for mat in (m, dp, dm):
        assert int(mat.colidx.max()) >= 1 << 31 and mat.nrows == sc.F.nrows
    assert sc.F.nrows < 4096 and sc.B.nrows < 8192                 # entry-sized: nothing here is as long as the key space


@pytest.mark.parametrize("N", me.KEY_SPACES + me.WIDE_KEY_SPACES)
def test_sort_cases_have_the_lengths_and_unique_counts_they_name(N):
    sc = me.sort_cases(N)
    names = {name for name, _, _ in sc.claims.values()}
    assert names == {f"L{L}-{p}" for L in me.SORT_LENGTHS for p in me.SORT_PATTERNS} | {f"dup{d}" for d in me.DUP_COUNTS}
    flen = sc.F.lengths()
    for i, (name, L, uniq) in sc.claims.items():
        seg = np.concatenate([sc.B.row(j) for j in sc.F.row(i).tolist()]).tolist()      # from F and B, not from the builder
        assert len(seg) == L == int(name.split("-")[0].lstrip("Ldup")), name
        assert flen[i] >= 2, name                                  # (more than one source: the sort runs)
        assert len(set(seg)) == uniq == len(sc.C.row(i)), name
        assert max(seg) < N
        if name.startswith("dup"):
            assert uniq == 1 and flen[i] == L
            continue
        a, b = (sc.B.row(j).tolist() for j in sc.F.row(i).tolist())
        pat = name.split("-")[1]
        if pat == "identical":
            assert uniq == (L + 1) // 2 and set(a) <= set(b) and len(b) - len(a) == L % 2
        else:
            assert uniq == min(L, N), name                         # disjoint, or the whole key space where L > N
        if pat == "below" and L <= N:
            assert max(b) < min(a)
        if pat == "interleave" and L <= N:
            assert all(x < y for x, y in zip(a, b)) and all(y < x for x, y in zip(a[1:], b))
        if pat == "ends":
            assert 0 in seg and N - 1 in seg
    # the classes interleave: a case row never follows a case row, and both fillers occur
    assert all(i + 1 not in sc.claims for i in sc.claims)
    fill = [i for i in range(sc.F.nrows) if i not in sc.claims]
    assert any(flen[i] == 0 for i in fill) and any(flen[i] == 1 for i in fill)
    assert (sc.F.nrows + 1) % 64 == 2
    classes = [0 if L <= 64 else 1 if L <= 4096 else 2 for _, L, _ in sc.claims.values()]
    assert {0, 1, 2} == set(classes)
    # the bitmap of the big class: a word count that is no multiple of 16 at the smallest key space
    assert ((me.KEY_SPACES[0] + 31) // 32) % 16 != 0


@pytest.mark.parametrize("N", me.KEY_SPACES)
def test_sort_case_references_agree_with_the_oracle(N):
    sc = me.sort_cases(N)
    same(sc.C, oracle.mxm(orc(sc.F), orc(sc.B))[0])
    r, c = sc.coo()
    assert len(r) >= 4096 and len(r) == sum(L for _, L, _ in sc.claims.values()) + sum(
        len(sc.segment(i)) for i in range(sc.F.nrows) if i not in sc.claims)
    same(sc.C, oracle.build_csr(sc.F.nrows, N, r, c))
    same(me.build(sc.F.nrows, N, r, c), oracle.build_csr(sc.F.nrows, N, r, c))
    m, dp, dm = sc.layers()
    for i, (name, L, _) in sc.claims.items():
        assert len(m.row(i)) + len(dp.row(i)) == (L if not name.startswith("dup") else 2), name
    assert dm.nnz > 0 and any(len(dm.row(i)) == 0 for i in sc.claims) and any(len(dm.row(i)) for i in sc.claims)
    for masks in (False, True):
        same(me.merge(m, dp, dm, masks), oracle.merge(orc(m), orc(dp), orc(dm), masks))
    same(me.merge(m, dp, None), oracle.merge(orc(m), orc(dp), None))
    assert me.merge(m, dp, None).nnz == sc.C.nnz                   # the same unions as the product's


@pytest.mark.parametrize("nrows", me.SCAN_NROWS)
def test_scan_cases_sit_on_the_tile_boundaries(nrows):
    assert (nrows + 1) in (4096, 4097, 4098, 8192, 8193, 8194)
    a, p, d, b = me.scan_case(nrows)
    live = set(np.nonzero(a.lengths())[0].tolist())
    assert {0, nrows - 1} <= live
    for t in range(me.SCAN_TILE, nrows + 1, me.SCAN_TILE):
        assert {t - 1, t} & set(range(nrows)) <= live
    assert len(live) <= 16 and a.nnz and p.nnz and d.nnz and b.nnz
    assert me.intersect(a, p).nnz and me.intersect(a, d).nnz and me.intersect(p, d).nnz
    for masks in (False, True):
        same(me.merge(a, p, d, masks), oracle.merge(orc(a), orc(p), orc(d), masks))
    same(me.mxm(a, b), oracle.mxm(orc(a), orc(b))[0])
    assert me.mxm(a, b).nnz
    same(me.transpose(a), oracle.transpose(orc(a)))
    assert me.intersect(a, p).to_set() == a.to_set() & p.to_set()
    assert me.resize(a, nrows - 2, 150).to_set() == {(r, c) for r, c in a.to_set() if r < nrows - 2 and c < 150}


def test_huge_case_needs_a_three_level_scan():
    assert me.HUGE_NROWS + 1 > me.SCAN_TILE ** 2
    a, b = me.huge_case()
    assert {0, 4095, 4096, (1 << 24) - 1, 1 << 24, me.HUGE_NROWS - 1} == set(a)
    sa = {(r, c) for r, cs in a.items() for c in cs}
    sb = {(r, c) for r, cs in b.items() for c in cs}
    assert 10 <= len(sa) <= 20 and 0 < len(sa & sb) < len(sb)
    rp, ci, hr = me.hyper_arrays(a)
    assert len(rp) == len(hr) + 1 and rp[-1] == len(ci) == len(sa)


@pytest.mark.parametrize("n", me.THRESHOLD_N)
def test_heavy_duplication_case(n):
    r, c, v = me.heavy_dup_coo(n)
    assert len(r) == n and len(set(v.tolist())) == n
    want = me.last_wins(r, c, v)
    assert len(want) <= 2500 < n
    same(me.build(50, 50, r, c), oracle.build_csr(50, 50, r, c))
    pos = {}
    for i, k in enumerate(zip(r.tolist(), c.tolist())):
        pos[k] = i
    assert all(want[k] == int(v[i]) for k, i in pos.items())


@pytest.mark.parametrize("ncols", me.TRANSPOSE_NCOLS)
@pytest.mark.parametrize("nnz", me.THRESHOLD_N)
def test_transpose_cases_hold_exactly_nnz_entries(nnz, ncols):
    nrows, r, c = me.transpose_case(nnz, ncols)
    assert len(r) == nnz == len(set(zip(r.tolist(), c.tolist())))
    assert int(r.max()) == nrows - 1 and int(c.max()) == ncols - 1 and int(r.min()) == 0 and int(c.min()) == 0
    a = me.build(nrows, ncols, r, c)
    same(a, oracle.build_csr(nrows, ncols, r, c))
    same(me.transpose(a), oracle.transpose(orc(a)))


@pytest.mark.parametrize("nrows,ncols", [(1, 70000), (70000, 1)])
def test_thin_cases(nrows, ncols):
    r, c = me.thin_case(nrows, ncols)
    a = me.build(nrows, ncols, r, c)
    assert len(r) == 6000 and a.nnz == 5000 >= 4096
    assert {0, max(nrows, ncols) - 1} <= set((r + c).tolist())
    same(a, oracle.build_csr(nrows, ncols, r, c))
    same(me.transpose(a), oracle.transpose(orc(a)))


def test_hyper_flip_cases():
    r, c = me.hyper_flip_coo(256)
    assert len(r) < 4096 and len(set(r.tolist())) == 256 and {0, 4095} <= set(r.tolist()) and int(c.max()) < 4096
    assert 256 * 16 <= 4097 and not 257 * 16 <= 4097              # the two sides of the rule at nrows = 4097
    r2, c2 = me.hyper_flip_coo(256, with_last_row=4096)
    assert len(set(r2.tolist())) == 257 and np.array_equal(r2[:len(r)], r) and np.array_equal(c2[:len(c)], c)
    assert me.build(4097, 4096, r, c).nnz == len(r)


def test_form_contents():
    x, y, z = (me.form_content(s) for s in (0, 1, 2))
    lens = set(x.lengths().tolist())
    assert {1, 63, 64, 65, 129} <= lens
    live = np.nonzero(x.lengths())[0]
    assert 24 <= len(live) <= 48 and {0, 4095, 4096, me.FORM_N - 1} <= set(live.tolist())
    assert len(live) * 16 <= me.FORM_N                             # few enough rows for the hypersparse form to be natural
    for a, b in ((x, y), (x, z), (y, z)):
        i = me.intersect(a, b)
        assert 0 < i.nnz < min(a.nnz, b.nnz)
        assert i.to_set() == a.to_set() & b.to_set()
    rp, hr = x.hyper()
    assert len(rp) == len(hr) + 1 == len(live) + 1 and rp[-1] == x.nnz
    same(me.mxm(x, y), oracle.mxm(orc(x), orc(y))[0])
    same(me.transpose(x), oracle.transpose(orc(x)))
    for masks in (False, True):
        same(me.merge(x, y, z, masks), oracle.merge(orc(x), orc(y), orc(z), masks))
    assert me.merge(x, y, z, False).nnz != me.merge(x, y, z, True).nnz
    v = me.value_of(*x.pairs())
    assert len(set(v.tolist())) == x.nnz
