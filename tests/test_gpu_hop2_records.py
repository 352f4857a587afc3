"""The mid-chain hop over a light state when records answer the flag probe (bitexpand.hip: bp_records_kernel writes a record
for EVERY vertex, bp_pull_groups_kernel<.., true> and bp_pull_items_rec_kernel read them behind the LDS flag map).

One constructed graph carries every case; its state after hop 1 is decided by the edges out of the sources, so which vertices
are flagged and how many bits each holds is read off the graph:

  - n = 3 * 2048 + 37: a records tile and a flag word both end part-way; vertex n - 1 is flagged and feeds a split row
  - split rows (more than 256 in-edges: the item kernel's) of in-degree 257, 300, 512 and 600, a group row of exactly 256
  - the 512 row's first item holds unflagged neighbours only, its second item flagged ones only; every other split row mixes
  - flagged vertices with exactly 1, 4, 5 and 17 bits (the record boundary and BP_REC_ESC), each feeding a split and a group row,
    with bits in the first and the last word of the row
  - unflagged neighbours next to a flagged vertex in their map block (they pass the map and must read ~0ull) and in blocks
    with none
  - hop 1 is light enough to be pushed, so hop 2 is the chain's one mid-chain pull: the profiler scopes asserted below are its

The second graph has the same shape on 2^24 + 5 vertices: a block of the 32 KiB map is then 128 vertices (cshift 7), two flag
words, where the base graph's is 8 (cshift 3, the smallest).  The map builder has one form for every shift, so these are its
two ends rather than two branches.
"""
import numpy as np
import pytest

import oracle
from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64

N_BASE = 3 * 2048 + 37
N_LARGE = (1 << 24) + 5
COARSE_LDS = 32 * 1024          # bitexpand.hip BP_COARSE_LDS
SRC0 = 2100
SPLIT = {10: 257, 1500: 300, 4000: 512, 4100: 600}     # destination -> in-degree
GROUP256 = 4200
SMALL = list(range(4201, 4231))                        # group rows of a few in-edges each
NO_IN_EDGE = 4300                                      # the destination of the dp entry
BITS = (1, 4, 5, 17)
ITEM_REC, RECORDS = "bp_pull_items_rec_kernel", "bp_records_kernel"


def coarse_shift(n):
    c = 3
    while (((n + (1 << c) - 1) >> c) + 63) // 64 * 8 > COARSE_LDS:
        c += 1
    return c


class Case:
    def __init__(self, n, nsrc):
        assert nsrc <= 1024 and n >= N_BASE
        self.n, self.nsrc = n, nsrc
        rng = np.random.default_rng(0xB17 + nsrc)
        self.src = np.arange(SRC0, SRC0 + nsrc, dtype=U64)
        p0 = self.p0 = (n - 581) & ~7
        top = np.arange(p0, n, dtype=I64)
        flagged = np.concatenate([[40, 41], top[top % 8 != 3]]).astype(I64)
        fp = np.concatenate([[42, 43], top[top % 8 == 3]]).astype(I64)          # unflagged, a flagged vertex in their block
        clear = np.setdiff1d(np.arange(64, 2048, dtype=I64), list(SPLIT))       # unflagged, no flagged vertex in their block
        special = {p0: [0], n - 1: [nsrc - 1], p0 + 1: [0, 1, nsrc - 2, nsrc - 1],
                   p0 + 2: [0, 1, 2, nsrc - 2, nsrc - 1], p0 + 4: [0] + list(range(nsrc - 16, nsrc))}
        assert [len(v) for v in special.values()] == [1, 1, 4, 5, 17] and set(special) <= set(flagged.tolist())
        pattern = (1, 4, 5, 17, 1, 2, 1, 3, 1, 1, 6, 1)
        er, ec = [], []
        for i, u in enumerate(flagged.tolist()):
            if u in special:
                who = special[u]
            else:
                c = pattern[i % len(pattern)]
                who = ((i * 37 + np.arange(c) * 3) % nsrc).tolist()
            assert len(set(who)) == len(who)
            er += [SRC0 + w for w in who]
            ec += [u] * len(who)
        sp = np.array(sorted(special), dtype=I64)
        rest = np.setdiff1d(flagged, sp)

        def into(v, n_clear, n_fp, n_flag, with_special=True):
            k = len(sp) if with_special else 0
            us = np.concatenate([rng.choice(clear, n_clear, replace=False), rng.choice(fp[2:], n_fp, replace=False),
                                 sp[:k], rng.choice(rest[2:], n_flag - k, replace=False)])
            assert len(np.unique(us)) == len(us)
            er.extend(us.tolist())
            ec.extend([v] * len(us))

        into(10, 126, 0, 131)
        into(1500, 150, 30, 120)
        # 4000: the 256 smallest in-neighbours (one item) are unflagged — 42 and 43 pass the map — and the other 256 flagged
        low = np.concatenate([[42, 43], rng.choice(clear, 254, replace=False)])
        high = np.concatenate([sp, rng.choice(rest[2:], 256 - len(sp), replace=False)])
        assert low.max() < high.min()
        er += low.tolist() + high.tolist()
        ec += [4000] * 512
        into(4100, 200, len(fp) - 2, 600 - 200 - (len(fp) - 2))
        into(GROUP256, 100, 20, 134)
        er += [40, 41]
        ec += [GROUP256] * 2
        for j, v in enumerate(SMALL):
            into(v, 1 + j % 7, j % 5, (len(sp) + 3) if j % 3 == 0 else 1 + j % 4, with_special=(j % 3 == 0))
        # out-edges of the hop-2 destinations (hop 3 has something to traverse) and unflagged filler that keeps hop 1 light
        fill_u = np.arange(3200, 4000, dtype=I64)
        dest = np.arange(4400, 5500, dtype=I64)
        for v in list(SPLIT) + [GROUP256] + SMALL + [NO_IN_EDGE]:
            d = rng.choice(dest, 6, replace=False)
            er += [v] * 6
            ec += d.tolist()
        fr = np.repeat(fill_u, 80)
        er += fr.tolist()
        ec += rng.choice(dest, len(fr)).tolist()
        self.a = oracle.build_csr(n, n, np.array(er, dtype=U64), np.array(ec, dtype=U64))
        self.dm = oracle.build_csr(n, n, np.array([n - 1], dtype=U64), np.array([4100], dtype=U64))       # out of a split row
        self.dp = oracle.build_csr(n, n, np.array([p0 + 4], dtype=U64), np.array([NO_IN_EDGE], dtype=U64))
        self.special = special
        self.check_shape()

    def check_shape(self):
        """The graph holds what the docstring says — from the graph itself, not from the library."""
        a, n = self.a, self.n
        rows, cols = (x.astype(I64) for x in a.pairs())
        indeg = np.bincount(cols, minlength=n)
        for v, d in SPLIT.items():
            assert indeg[v] == d
        assert indeg[GROUP256] == 256 and indeg[NO_IN_EDGE] == 0
        assert a.has_edges([n - 1], [4100])[0] and not a.has_edges([self.p0 + 4], [NO_IN_EDGE])[0]
        is_src = np.zeros(n, dtype=bool)
        is_src[self.src.astype(I64)] = True
        assert not is_src[cols].any()                       # no source is reached: hop 1's state is the sources' out-edges
        from_src = is_src[rows]
        cnt = np.bincount(cols[from_src], minlength=n)      # bits of X[u] after hop 1 (the sources' edges are distinct)
        for u, who in self.special.items():
            assert cnt[u] == len(who)
        assert set(BITS) <= set(cnt[list(self.special)].tolist())
        flagged = cnt > 0
        assert flagged[n - 1] and flagged.sum() * 8 < n     # the sparse form
        T = int(from_src.sum())
        assert T * 32 <= a.nnz                              # hop 1 is pushed
        cs = coarse_shift(n)
        assert cs == (3 if n == N_BASE else 7)
        block = np.zeros((n >> cs) + 1, dtype=bool)
        block[np.flatnonzero(flagged) >> cs] = True
        u, v = rows[~from_src], cols[~from_src]
        split = indeg[v] > 256
        kinds = {"record": (cnt[u] >= 1) & (cnt[u] <= 4), "esc": cnt[u] > 4, "false positive": ~flagged[u] & block[u >> cs],
                 "rejected by the map": ~block[u >> cs]}
        for name, k in kinds.items():
            assert (k & split).any() and (k & ~split).any(), name
        # the 512 row: one item all unflagged, one all flagged; the other split rows mix inside their first item
        at = oracle.transpose(a)
        ins = at.row(4000).astype(I64)
        assert not flagged[ins[:256]].any() and flagged[ins[256:]].all()
        for v in (10, 1500, 4100):
            first = flagged[at.row(v).astype(I64)[:256]]
            assert first.any() and not first.all()
        for who in self.special.values():                   # bits in the first and the last word of the row
            assert min(who) < 64 or max(who) >= self.nsrc - 64
        assert any(0 in who for who in self.special.values()) and any(self.nsrc - 1 in who for who in self.special.values())

    def refs(self):
        if not hasattr(self, "_refs"):
            clean = [(self.a, None, None)]
            dirty = [(self.a, self.dp, self.dm)]
            self._refs = {"mat": oracle.expand_omp(self.src, clean * 2)[:2],
                          "count": oracle.expand_summary_omp(self.src, clean * 3, chunk=1024)[:3],
                          "count dirty": oracle.expand_summary_omp(self.src, dirty * 3, chunk=1024)[:3]}
            assert self._refs["count"] != self._refs["count dirty"]
        return self._refs

    def device(self, ctx):
        if not hasattr(self, "_dev"):
            coo = lambda m: ctx.mat_from_coo(m.nrows, m.ncols, *m.pairs())
            self._dev = tuple(coo(m) for m in (self.a, self.dp, self.dm))
        return self._dev

    def free(self):
        for m in getattr(self, "_dev", ()):
            m.free()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, nsrc):
        if (n, nsrc) not in made:
            made[(n, nsrc)] = Case(n, nsrc)
        return made[(n, nsrc)]

    yield get
    for c in made.values():
        c.free()


class Forced:
    def __init__(self, ctx, **opts):
        self.ctx, self.opts, self.found = ctx, dict(expand_mode=2, expand_xcd_min_mb=0, **opts), {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.found[k] = self.ctx.get_option(k)
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in reversed(list(self.found.items())):
            self.ctx.set_option(k, v)


def run(ctx, records, call):
    """call() under the forced path with expand_records = records; the launches by profiler scope next to its result."""
    with Forced(ctx, expand_records=records):
        ctx.prof_enable(True)
        try:
            out = call()
            launches = {p["kernel"]: p["launches"] for p in ctx.prof_read()}
        finally:
            ctx.prof_enable(False)
    print("records", records, {k: v for k, v in launches.items() if k in (ITEM_REC, RECORDS)})
    if records:
        assert launches.get(ITEM_REC, 0) >= 1 and launches.get(RECORDS, 0) >= 1, sorted(launches)
    else:
        assert ITEM_REC not in launches and RECORDS not in launches, sorted(launches)
    return out


def materialised(ctx, case, records):
    a, _, _ = case.device(ctx)

    def call():
        m, flops = engine.expand_mat(ctx, case.src, [a] * 2)
        rp, ci, _ = m.export_csr()
        m.free()
        return np.asarray(rp).astype(U64), np.asarray(ci).astype(U64), flops

    return run(ctx, records, call)


SHAPES = [(N_BASE, 64), (N_BASE, 128), (N_BASE, 256), (N_BASE, 512), (N_BASE, 1024), (N_LARGE, 64)]


@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_two_hops_materialised(ctx, cases, n, nsrc):
    case = cases(n, nsrc)
    want, want_flops = case.refs()["mat"]
    got = {r: materialised(ctx, case, r) for r in (1, 0)}
    for r, (rp, ci, flops) in got.items():
        assert np.array_equal(rp, want.rowptr.astype(U64)), r
        assert np.array_equal(ci, want.colidx.astype(U64)), r
        assert flops == want_flops, r
    assert all(np.array_equal(x, y) for x, y in zip(got[1][:2], got[0][:2]))


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_three_hops_counted(ctx, cases, n, nsrc, dirty):
    case = cases(n, nsrc)
    want = case.refs()["count dirty" if dirty else "count"]
    a, dp, dm = case.device(ctx)
    layers = ([a] * 3, [dp] * 3, [dm] * 3) if dirty else ([a] * 3,)
    got = {r: run(ctx, r, lambda: engine.expand_count(ctx, case.src, *layers)) for r in (1, 0)}
    assert got[1] == tuple(want), (got[1], want)
    assert got[0] == tuple(want), (got[0], want)
