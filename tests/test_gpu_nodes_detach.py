"""fgpu_nodes_detach (csrc/detach.hip): a node set leaves a matrix and its transposed pattern, the removal list comes back in the
reference's order.  The checker is tests/detach_check.py's detach_matrix — dicts and sorted() — and every output matrix is read
back whole with fgpu_mat_export_csr.  Shapes are the smallest at which a pass can go wrong: a bitmap with a tail word, more than
one 256-lane workgroup, scans over several blocks, one row longer than a workgroup, a hypersparse input."""
import gc
import os
import sys

import numpy as np
import pytest

from falkordb_amd import _ffi, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_edges as me  # noqa: E402
from detach_check import MULTI, detach_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64


def split(entries):
    k = sorted(entries)
    return (np.array([r for r, _ in k], dtype=U64), np.array([c for _, c in k], dtype=U64),
            np.array([entries[x] for x in k], dtype=U64))


def build(ctx, nrows, ncols, entries, valued=True, hyper=False):
    """(m, mt): the matrix of `entries` — valued or BOOL, in the hypersparse form when asked — and its BOOL transposed pattern."""
    r, c, v = split(entries)
    if hyper:
        a = me.build(nrows, ncols, r, c)
        rp, hr = a.hyper()
        m = ctx.mat_from_csr(nrows, ncols, rp, a.colidx, vals=v if valued else None, hyper_rows=hr)
    else:
        m = ctx.mat_from_coo(nrows, ncols, r, c, v if valued else None)
    return m, ctx.mat_from_coo(ncols, nrows, c, r)


def assert_matrix(mat, nrows, ncols, kept, valued):
    """mat == the entries `kept`, row by row, through the full export"""
    assert (mat.nrows, mat.ncols, mat.nvals, mat.has_values) == (nrows, ncols, len(kept), valued)
    r, c, v = split(kept)
    rp, ci, vals = mat.export_csr()
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(r.astype(np.int64), minlength=nrows))]).astype(U64))
    assert np.array_equal(ci, c)
    if valued:
        assert vals is not None and np.array_equal(vals, v)
    else:
        assert vals is None


def check(ctx, nrows, ncols, entries, nodes, sides=3, valued=True, hyper=False, with_mt=True, want_list=True):
    """One call held against detach_matrix in everything it returns; returns the stats."""
    m, mt = build(ctx, nrows, ncols, entries, valued, hyper)
    if not valued:
        entries = dict.fromkeys(entries, 0)
    kept, out, inn, want_st = detach_matrix(entries, nodes, sides)
    mo, mto, rr, rc, rv, n_out, st = engine.nodes_detach(ctx, m, mt if with_mt else None, nodes, sides, want_list=want_list,
                                                         stats=True)
    assert_matrix(mo, nrows, ncols, kept, valued)
    if with_mt:
        assert_matrix(mto, ncols, nrows, {(c, r): 0 for r, c in kept}, False)
    else:
        assert mto is None
        want_st[5] = 0
    got = list(zip(rr.tolist(), rc.tolist(), rv.tolist()))
    if want_list:
        assert n_out == len(out) and got[:n_out] == out and got[n_out:] == inn
    else:
        assert got == [] and n_out == 0
        want_st[1] = want_st[2] = 0
    if not valued:
        want_st[3] = 0
    assert st[:6] == want_st and st[6:] == [0, 0]
    assert_matrix(m, nrows, ncols, entries, valued)                      # the inputs are untouched
    return st


def multigraph_entries(seed, n, count, ncols=None):
    """`count` distinct coordinates of an n x ncols matrix; about a quarter carry MULTI, the others a distinct id with high bits."""
    rng = np.random.default_rng(seed)
    ncols = n if ncols is None else ncols
    lin = rng.choice(n * ncols, count, replace=False)
    ent = {}
    for k, x in enumerate(lin.tolist()):
        ent[(x // ncols, x % ncols)] = MULTI if k % 4 == 0 else (1 << 40) + 7 * k
    return ent


@pytest.fixture(scope="module")
def big():
    return multigraph_entries(5000, 5000, 40000)


def test_tail_word_and_one_workgroup_crossed(ctx):
    """n = 300 (the bitmap ends inside a word), 3000 entries (12 workgroups), |D| = 37, MULTI values among the removed."""
    ent = multigraph_entries(300, 300, 3000)
    D = np.r_[np.random.default_rng(37).choice(299, 36, replace=False), [299]]   # (the last node: the last bit of the tail word)
    st = check(ctx, 300, 300, ent, D)
    assert st[0] == 37 and st[1] > 0 and st[2] > 0 and st[3] > 0 and 0 < st[4] < 3000


@pytest.mark.parametrize("which", ["none", "one", "all"])
def test_scans_over_several_blocks(ctx, big, which):
    """n = 5000, 40 000 entries.  D empty: copies and an empty list; D = everything: empty outputs, every entry listed once."""
    D = {"none": [], "one": [1234], "all": np.arange(5000)}[which]
    st = check(ctx, 5000, 5000, big, D)
    if which == "none":
        assert st[:6] == [0, 0, 0, 0, 40000, 40000]
    if which == "all":
        assert st[1] == 40000 and st[2] == 0 and st[4] == 0 and st[5] == 0


@pytest.mark.parametrize("hub_deleted", [True, False], ids=["hub-in-D", "hub-survives"])
def test_a_hub_row_longer_than_a_workgroup(ctx, hub_deleted):
    """Node 777 of 6000 holds 5000 out and 5000 in entries: one row of m and one of mt span twenty workgroups."""
    n, hub = 6000, 777
    rng = np.random.default_rng(6000)
    ent = multigraph_entries(6001, n, 3000)
    for k, v in enumerate(rng.choice(n, 5000, replace=False).tolist()):
        ent[(hub, v)] = MULTI if k % 5 == 0 else 10**12 + k
    for k, v in enumerate(rng.choice(n, 5000, replace=False).tolist()):
        ent.setdefault((v, hub), 2 * 10**12 + k)
    nbrs = sorted({c for r, c in ent if r == hub} | {r for r, c in ent if c == hub})
    D = [hub, 5, 5999] if hub_deleted else [x for x in nbrs if x != hub][::7]
    st = check(ctx, n, n, ent, D)
    if hub_deleted:
        assert st[1] >= 5000 and st[2] >= 4900
    else:
        assert st[1] > 0 and st[2] > 0 and st[4] > 3000


def test_a_hypersparse_input(ctx):
    """matrix_edges.form_content: 36 populated rows of 5000 — below the builders' hypersparse threshold, which the assert
    restates — stored with hyper_rows, and the same content through fgpu_mat_from_coo.  D names stored rows, empty rows and
    nodes that occur as columns; then every stored row (no row is left), then empty rows only, without transpose and list."""
    a = me.form_content(0)
    r, c = a.pairs()
    ent = {(int(x), int(y)): (MULTI if k % 3 == 0 else 5 * 10**10 + k) for k, (x, y) in enumerate(zip(r, c))}
    stored = sorted({x for x, _ in ent})
    assert len(stored) * 16 <= me.FORM_N and me.FORM_N > 4096
    empty = [x for x in range(me.FORM_N) if x not in set(stored)]
    D = stored[::5] + empty[:3] + [empty[-1]] + sorted({y for _, y in ent})[:40]
    for hyper in (True, False):
        st = check(ctx, me.FORM_N, me.FORM_N, ent, D, hyper=hyper)
        assert st[1] > 0 and st[2] > 0 and st[4] > 0
    check(ctx, me.FORM_N, me.FORM_N, ent, stored, hyper=True)             # every stored row goes: an empty hypersparse result
    check(ctx, me.FORM_N, me.FORM_N, ent, empty[:50], hyper=True, with_mt=False, want_list=False)


def test_rows_only_on_a_label_matrix_and_no_list_on_an_adjacency(ctx):
    """sides = 1 on a non-square 300 x 64 BOOL matrix (node x label), with and without its transpose; sides = 3 on a square
    BOOL matrix without list and without transpose (the adjacency)."""
    lab = dict.fromkeys(multigraph_entries(64, 300, 2500, ncols=64), 0)
    D = np.random.default_rng(1).choice(300, 80, replace=False)            # ids past 64: rows only, never read as columns
    st = check(ctx, 300, 64, lab, D, sides=1, valued=False, with_mt=False, want_list=False)
    assert 0 < st[4] < 2500
    check(ctx, 300, 64, lab, D, sides=1, valued=False, want_list=False)
    check(ctx, 300, 64, lab, D, sides=1, valued=False)                     # ... with the list: out entries only
    adj = dict.fromkeys(multigraph_entries(65, 300, 3000), 0)
    check(ctx, 300, 300, adj, D, sides=3, valued=False, with_mt=False, want_list=False)
    check(ctx, 300, 300, adj, D, sides=3, valued=False)
    check(ctx, 300, 300, multigraph_entries(66, 300, 3000), D, sides=2)    # columns only: every removed entry is an in entry


def test_node_order_and_duplicates_do_not_matter(ctx):
    ent = multigraph_entries(301, 300, 3000)
    m, mt = build(ctx, 300, 300, ent)
    D = np.random.default_rng(2).choice(300, 50, replace=False)
    messy = np.random.default_rng(3).permutation(np.r_[D, D[:20], D[:5]])

    def plain(res):
        mo, mto, rr, rc, rv, n_out, st = res
        return ([x.tolist() for x in mo.export_csr()], [x.tolist() for x in mto.export_csr()[:2]], rr.tolist(), rc.tolist(),
                rv.tolist(), n_out, st)
    assert plain(engine.nodes_detach(ctx, m, mt, np.sort(D), stats=True)) == plain(engine.nodes_detach(ctx, m, mt, messy, stats=True))


def test_self_loops(ctx):
    """A loop on a deleted node is an out entry and nothing else; a loop on a surviving node stays."""
    ent = multigraph_entries(302, 300, 2000)
    for v in (3, 64, 299, 100, 101):
        ent[(v, v)] = 9000 + v
    st = check(ctx, 300, 300, ent, [3, 64, 299, 7])
    m, mt = build(ctx, 300, 300, ent)
    mo, mto, rr, rc, rv, n_out = engine.nodes_detach(ctx, m, mt, [3, 64, 299, 7])
    loops = [(a, b, v) for a, b, v in zip(rr.tolist(), rc.tolist(), rv.tolist()) if a == b]
    assert loops == [(3, 3, 9003), (64, 64, 9064), (299, 299, 9299)] and all(k < n_out for k in range(len(rr)) if rr[k] == rc[k])
    assert mo.probe([100, 101, 3], [100, 101, 3]).tolist() == [1, 1, 0] and st[1] >= 3


def _raises_invalid(fn):
    with pytest.raises(_ffi.FgpuError) as e:
        fn()
    assert e.value.code == _ffi.FGPU_INVALID
    assert str(e.value).split(":", 1)[1].strip()   # fgpu_last_error is set


def test_rejections_leave_the_context_usable(ctx):
    ent = multigraph_entries(303, 300, 2000)
    m, mt = build(ctx, 300, 300, ent)
    rect, rect_t = build(ctx, 300, 64, dict.fromkeys(multigraph_entries(67, 300, 500, ncols=64), 0), valued=False)
    valued_t = ctx.mat_from_coo(300, 300, [1], [2], [3])
    cases = [
        lambda: engine.nodes_detach(ctx, m, mt, [300]),                                  # a node at the dimension
        lambda: engine.nodes_detach(ctx, m, mt, [5, 2**40]),
        lambda: engine.nodes_detach(ctx, rect, rect_t, [64], sides=2, want_list=False),  # ... at the COLUMN dimension it indexes
        lambda: engine.nodes_detach(ctx, m, mt, [5], sides=0),                           # sides outside 1..3
        lambda: engine.nodes_detach(ctx, m, mt, [5], sides=4),
        lambda: engine.nodes_detach(ctx, rect, rect_t, [5], sides=3),                    # a list over both sides, not square
        lambda: engine.nodes_detach(ctx, m, rect_t, [5]),                                # mt of other dimensions
        lambda: engine.nodes_detach(ctx, m, valued_t, [5]),                              # mt valued
        lambda: engine.nodes_detach(ctx, m, None, [5]),                                  # a list without mt
    ]
    ctx.sync()
    for bad in cases:
        before = ctx.device_bytes()[0]
        _raises_invalid(bad)
        ctx.sync()
        assert ctx.device_bytes()[0] == before, "a rejected call keeps device memory"
        check(ctx, 300, 300, ent, [5, 6])                                                # the next call is exact
    engine.nodes_detach(ctx, rect, rect_t, [64, 299], sides=1, want_list=False)          # 64 is a row here: accepted


def test_a_call_keeps_no_device_memory(ctx):
    """As tests/test_gpu_expand_ownership.py: warm, read in_use, call again, free what came back — in_use is where it was."""
    ent = multigraph_entries(304, 5000, 20000)
    m, mt = build(ctx, 5000, 5000, ent)
    D = np.arange(0, 5000, 9)

    def call():
        res = engine.nodes_detach(ctx, m, mt, D, stats=True)
        plain = (res[0].nvals, res[1].nvals, res[2].tolist(), res[3].tolist(), res[4].tolist(), res[5], res[6])
        res[0].free()
        res[1].free()
        del res
        gc.collect()
        return plain
    first = call()
    ctx.sync()
    in_use = ctx.device_bytes()[0]
    second = call()
    ctx.sync()
    assert ctx.device_bytes()[0] == in_use and second == first
