"""The mid-chain hop over the packed item stream (bitexpand.hip: bp_group_items cuts the rows of at most 256 entries of A' into
items once per snapshot, bp_pull_groups_kernel<.., true, true> takes a wavefront per item; option expand_group_items).

The graph is the constructed one of tests/hop_graph.py (split rows of 257 / 300 / 512 / 600 in-edges, a row of exactly 256,
flagged neighbours of 1 / 4 / 5 / 17 bits, map false positives, vertex n - 1 flagged and fed by the sources) with the rows the
cut rule turns on added to it; where the items begin and end is asserted below from the index read back, not assumed:

  - row 4200, 256 in-edges, alone in its item
  - rows 4001 .. 4031 hold 255 entries, row 4032 two: the item is closed by entries, before its 32nd row
  - rows 4150 .. 4182 hold one entry each: the first item is closed by rows, at 32
  - split row 10 between the one-entry rows 9 and 11, split row 4100 between 4099 and 4101: split rows INSIDE an item (they count
    zero); split rows 1500 and 4000 have no short neighbour within 32 rows: between items
  - more than 64 consecutive empty rows between two items
  - the last item ends at row n - 1
  - a dp entry into row 4160 and a dm entry out of row 4005's in-edges: rows that are summed later, in items whose first row is
    not a multiple of 64 (item 4150 .. 4181 reads its 32 `later` bits from two words of the bitmap)

The same shape on 2^24 + 5 vertices has a 128-vertex map block (cshift 7) and item headers far apart.
"""
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hop_graph import GROUP256, N_BASE, N_LARGE, SPLIT, Case, Forced  # noqa: E402

ITEM, ROWS = 256, 32
BY_ENTRIES = (4001, 31, 255)      # (first row, rows, entries) of the item closed by entries; row 4032 holds 2
BY_ROWS = (4150, 32, 32)          # ... closed by rows; row 4182 holds one more
DP_ROW, DM_ROW = 4160, 4005
COUNTER = "expand_group_item_launches"


class ItemCase(Case):
    def __init__(self, n, nsrc):
        super().__init__(n, nsrc)
        self.a_base = self.a
        k, p0 = self.k, self.p0
        top = np.arange(p0, n, dtype=I64)
        fp = top[top % 8 == 3]                                        # unflagged, flagged vertices in their map block
        clear = np.setdiff1d(np.arange(64, 2048, dtype=I64), list(SPLIT))
        sp = np.array(sorted(self.special), dtype=I64)                # 1 / 1 / 4 / 5 / 17 bits
        rest = np.setdiff1d(top[top % 8 != 3], sp)                    # the other flagged vertices
        er, ec = [], []

        def into(v, us):
            assert len(set(us)) == len(us)
            er.extend(int(u) for u in us)
            ec.extend([v] * len(us))

        for j, v in enumerate((9, 11, 4099, 4101)):
            into(v, [sp[j]])
        for j in range(31):                                           # 30 rows of 8 and one of 15: 255
            us = [sp[j % 5], fp[j], rest[2 * j], rest[2 * j + 1]] + clear[8 * j:8 * j + 4].tolist()
            if j == 30:
                us += clear[400:407].tolist()
            into(BY_ENTRIES[0] + j, us)
        into(4032, [sp[4], clear[500]])
        for j in range(33):
            into(BY_ROWS[0] + j, [(sp[j % 5], fp[40 + j], clear[600 + j])[j % 3]])
        dest = np.arange(4400, 5500, dtype=I64)
        for j, v in enumerate(sorted(set(ec))):                       # hop 3 has something to traverse out of the new rows
            into_v = dest[(j * 17) % len(dest)], dest[(j * 17 + 5) % len(dest)]
            er.extend([v, v])
            ec.extend(int(d) for d in into_v)
        r0, c0 = self.a_base.pairs()
        self.a = oracle.build_csr(n, n, np.concatenate([r0, np.array(er, dtype=U64)]), np.concatenate([c0, np.array(ec, dtype=U64)]))
        assert self.a.nnz == self.a_base.nnz + len(er)
        self.check_shape()
        # the delta layers: the base graph's entries and one of each into a short row inside an item
        dm_u = int(oracle.transpose(self.a).row(DM_ROW)[0])
        self.dm = oracle.build_csr(n, n, np.array([n - 1, dm_u], dtype=U64), np.array([4100, DM_ROW], dtype=U64))
        self.dp = oracle.build_csr(n, n, np.array([p0 + 4, p0 + 1], dtype=U64), np.array([4300, DP_ROW], dtype=U64))
        assert self.a.has_edges([n - 1, dm_u], [4100, DM_ROW]).all() and not self.a.has_edges([p0 + 4, p0 + 1], [4300, DP_ROW]).any()
        if hasattr(self, "_refs"):
            del self._refs

    def refs(self):
        if not hasattr(self, "_refs"):
            super().refs()
            mixed = [(self.a, None, None), (self.a, None, None), (self.a_base, None, None)]
            self._refs["count mixed"] = oracle.expand_summary_omp(self.src, mixed, chunk=1024)[:3]
            assert self._refs["count mixed"] != self._refs["count"]
        return self._refs

    def device(self, ctx):
        if not hasattr(self, "_dev"):
            super().device(ctx)
            self._dev_base = ctx.mat_from_coo(self.n, self.n, *self.a_base.pairs())
        return self._dev

    def free(self):
        super().free()
        if hasattr(self, "_dev_base"):
            self._dev_base.free()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, nsrc):
        if (n, nsrc) not in made:
            made[(n, nsrc)] = ItemCase(n, nsrc)
        return made[(n, nsrc)]

    yield get
    for c in made.values():
        c.free()


def run(ctx, form, call):
    """call() with expand_group_items = form on the forced bit-parallel path; the launch counter says which form ran."""
    with Forced(ctx, expand_group_items=form):
        before = ctx.get_option(COUNTER)
        out = call()
        ran = ctx.get_option(COUNTER) - before
    print("expand_group_items", form, "packed launches", ran)
    assert (ran >= 1) if form else (ran == 0), (form, ran)
    return out


SHAPES = [(n, nsrc) for n in (N_BASE, N_LARGE) for nsrc in (64, 512, 1024)]


@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_two_hops_materialised(ctx, cases, n, nsrc):
    case = cases(n, nsrc)
    want, want_flops = case.refs()["mat"]
    a, _, _ = case.device(ctx)

    def call():
        m, flops = engine.expand_mat(ctx, case.src, [a] * 2)
        rp, ci, _ = m.export_csr()
        m.free()
        return np.asarray(rp).astype(U64), np.asarray(ci).astype(U64), flops

    got = {f: run(ctx, f, call) for f in (1, 0)}
    for f, (rp, ci, flops) in got.items():
        assert np.array_equal(rp, want.rowptr.astype(U64)), f
        assert np.array_equal(ci, want.colidx.astype(U64)), f
        assert flops == want_flops, f
    assert all(np.array_equal(x, y) for x, y in zip(got[1][:2], got[0][:2]))


@pytest.mark.parametrize("layers", ["clean", "dirty", "mixed"])
@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_three_hops_counted(ctx, cases, n, nsrc, layers):
    case = cases(n, nsrc)
    want = case.refs()[{"clean": "count", "dirty": "count dirty", "mixed": "count mixed"}[layers]]
    a, dp, dm = case.device(ctx)
    args = {"clean": ([a] * 3,), "dirty": ([a] * 3, [dp] * 3, [dm] * 3), "mixed": ([a, a, case._dev_base],)}[layers]
    for f in (1, 0):
        got = run(ctx, f, lambda: engine.expand_count(ctx, case.src, *args))
        assert got == tuple(want), (f, got, want)


def test_cut_rule(ctx, cases):
    """The index read back for the small graph: whole rows, at most 32 rows and 256 entries, every entry of a short row exactly
    once under its row bits, the greedy cut in vertex order, and the items the docstring names."""
    case = cases(N_BASE, 64)
    n = case.n
    a, _, _ = case.device(ctx)
    hdr, cols = a.group_items()
    hdr, cols = np.asarray(hdr).astype(I64), np.asarray(cols)
    at = oracle.transpose(case.a)
    deg = np.diff(at.rowptr.astype(I64))
    short = np.where(deg <= ITEM, deg, 0)
    v0, r, cnt = hdr[:, 0], hdr[:, 1], hdr[:, 2]
    assert (hdr[:, 3] == 0).all() and (r >= 1).all() and (r <= ROWS).all() and (cnt >= 1).all() and (cnt <= ITEM).all()
    assert (v0[1:] >= v0[:-1] + r[:-1]).all() and v0[-1] + r[-1] == n            # disjoint, ascending, the last one ends at n - 1
    covered = np.zeros(n, dtype=bool)
    got_rows, got_cols = [], []
    for i in range(len(hdr)):
        covered[v0[i]:v0[i] + r[i]] = True
        assert short[v0[i]:v0[i] + r[i]].sum() == cnt[i]                         # whole rows
        assert short[v0[i]] > 0 and short[v0[i] + r[i] - 1] > 0                  # begins and ends on a row that holds entries
        w = cols[i]
        assert (w[cnt[i]:] == 0xFFFFFFFF).all() and (w[:cnt[i]] != 0xFFFFFFFF).all()
        got_rows.append(v0[i] + (w[:cnt[i]] >> 27).astype(I64))
        got_cols.append((w[:cnt[i]] & ((1 << 27) - 1)).astype(I64))
    assert not short[~covered].any()
    got_rows, got_cols = np.concatenate(got_rows), np.concatenate(got_cols)
    assert (np.diff(got_rows) >= 0).all()                                        # rows in order inside an item and across items
    rows_t = np.repeat(np.arange(n, dtype=I64), deg)
    keep = short[rows_t] > 0
    assert np.array_equal(got_rows, rows_t[keep]) and np.array_equal(got_cols, at.colidx.astype(I64)[keep])
    # the greedy cut, replayed
    want, v = [], 0
    while v < n:
        if short[v] == 0:
            v += 1
            continue
        b, c, last = v, 0, v
        while v < n and v - b < ROWS and c + short[v] <= ITEM:
            c += short[v]
            if short[v]:
                last = v
            v += 1
        want.append((b, last - b + 1, c))
    assert [tuple(x) for x in hdr[:, :3].tolist()] == want
    # the items this graph was built for
    items = {int(x[0]): (int(x[1]), int(x[2])) for x in hdr}
    assert items[GROUP256] == (1, 256)
    assert items[BY_ENTRIES[0]] == BY_ENTRIES[1:] and short[BY_ENTRIES[0] + BY_ENTRIES[1]] == 2
    assert items[BY_ROWS[0]] == BY_ROWS[1:] and short[BY_ROWS[0] + ROWS] == 1 and BY_ROWS[0] + ROWS in items
    inside = lambda s: bool(((v0 < s) & (s < v0 + r - 1)).any())
    assert inside(10) and inside(4100) and not covered[1500] and not covered[4000]
    assert (deg[[10, 1500, 4100]] == [257, 300, 600]).all()
    assert (v0[1:] - (v0[:-1] + r[:-1])).max() > 64                              # more than 64 empty rows between two items
    for d in (DP_ROW, DM_ROW):
        i = int(np.flatnonzero((v0 <= d) & (d < v0 + r))[0])
        assert v0[i] % 64 != 0 and 0 < short[d] <= ITEM
    i = int(np.flatnonzero(v0 == BY_ROWS[0])[0])
    assert v0[i] // 64 != (v0[i] + r[i] - 1) // 64                               # its `later` bits come from two words
