"""The constructed graph of the hop tests (test_gpu_hop2_records.py, test_gpu_hop_paths.py) and the option guard they share.

One graph carries every case; its state after hop 1 is decided by the edges out of the sources, so which vertices are flagged
and how many bits each holds is read off the graph.  test_gpu_hop2_records.py describes what the base graph holds; `heavy`
and `cover` below are the variants test_gpu_hop_paths.py adds, and 2048 sources its widest row.
"""
import numpy as np

import oracle

U64, I64 = np.uint64, np.int64

N_BASE = 3 * 2048 + 37
N_LARGE = (1 << 24) + 5
COARSE_LDS = 32 * 1024          # bitexpand.hip BP_COARSE_LDS
SRC0 = 2100
SPLIT = {10: 257, 1500: 300, 4000: 512, 4100: 600}     # destination -> in-degree
GROUP256 = 4200
SMALL = list(range(4201, 4231))                        # group rows of a few in-edges each
NO_IN_EDGE = 4300                                      # the destination of the dp entry
HEAVY_SPLIT = 4231                                     # heavy variant: a 600-entry row of hop 3
BITS = (1, 4, 5, 17)
ITEM_REC, RECORDS = "bp_pull_items_rec_kernel", "bp_records_kernel"


def coarse_shift(n):
    c = 3
    while (((n + (1 << c) - 1) >> c) + 63) // 64 * 8 > COARSE_LDS:
        c += 1
    return c


class Case:
    def __init__(self, n, nsrc, heavy=False, cover=False):
        """heavy: the sources also reach every filler vertex, so the states after hop 1 and hop 2 hold >= n / 8 non-zero rows (the
        dense forms), and the rows of the latter have out-edges for hop 3 to gather them by; cover: a source without an out-edge gets one, so no source row is compacted away and the rows are
        ceil(nsrc / 64) words wide.  nsrc = 2048: sources 1024.. are the first 1024 `clear` vertices, which have out-edges (into
        the split and group rows) and no in-edge; the pattern below stays on the first k = 1024."""
        assert (nsrc <= 1024 or nsrc == 2048) and n >= N_BASE and (n == N_BASE or not (heavy or cover or nsrc > 1024))
        self.n, self.nsrc, self.heavy, self.cover = n, nsrc, heavy, cover
        rng = np.random.default_rng(0xB17 + nsrc)
        k = self.k = min(nsrc, 1024)
        p0 = self.p0 = (n - 581) & ~7
        top = np.arange(p0, n, dtype=I64)
        flagged = np.concatenate([[40, 41], top[top % 8 != 3]]).astype(I64)
        fp = np.concatenate([[42, 43], top[top % 8 == 3]]).astype(I64)          # unflagged, a flagged vertex in their block
        clear = np.setdiff1d(np.arange(64, 2048, dtype=I64), list(SPLIT))       # unflagged, no flagged vertex in their block
        self.src = np.concatenate([np.arange(SRC0, SRC0 + k), clear[:nsrc - k]]).astype(U64)
        special = {p0: [0], n - 1: [k - 1], p0 + 1: [0, 1, k - 2, k - 1],
                   p0 + 2: [0, 1, 2, k - 2, k - 1], p0 + 4: [0] + list(range(k - 16, k))}
        assert [len(v) for v in special.values()] == [1, 1, 4, 5, 17] and set(special) <= set(flagged.tolist())
        pattern = (1, 4, 5, 17, 1, 2, 1, 3, 1, 1, 6, 1)
        er, ec = [], []
        for i, u in enumerate(flagged.tolist()):
            if u in special:
                who = special[u]
            else:
                c = pattern[i % len(pattern)]
                who = ((i * 37 + np.arange(c) * 3) % k).tolist()
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
        if heavy:
            for j, u in enumerate(fill_u.tolist()):
                for w in {j % nsrc, (j * 7 + 3) % nsrc}:
                    er.append(int(self.src[w]))
                    ec.append(u)
            # ... and the rows of the state after hop 2 (the hop-3 sources below) are gathered by hop 3, into 99 vertices nothing
            # else names: 40 of them with ONE in-edge (the row itself comes out, not an OR that fills up), the others with ~70,
            # and 600 into one more row that is cut into items
            sink = np.arange(4301, 4400, dtype=I64)
            for j, d in enumerate(dest.tolist()):
                er += [d] * (1 if j < 40 else 4)
                ec += [int(sink[j])] if j < 40 else [int(sink[40 + (j * 5 + q * 13) % 59]) for q in range(4)]
            er += dest[:600].tolist()
            ec += [HEAVY_SPLIT] * 600
        if cover:
            dead = np.setdiff1d(self.src.astype(I64), np.array(er, dtype=I64))
            er += dead.tolist()
            ec += [40] * len(dead)
        if heavy or cover:
            # hop 1 stays light enough to be pushed (T * 32 <= nnz): filler out of vertices that nothing reaches
            is_src = np.isin(np.array(er, dtype=I64), self.src.astype(I64))
            pairs = len(set(zip(er, ec)))
            need = 32 * int(is_src.sum()) - pairs + 64
            pad = np.arange(5500, 5600, dtype=I64)
            per = max(0, -(-need // len(pad)))
            assert per <= len(dest) and pad.max() < p0
            for v in pad.tolist():
                er += [v] * per
                ec += rng.choice(dest, per, replace=False).tolist()
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
        assert flagged[n - 1] and (flagged.sum() * 8 >= n + 16 if self.heavy else flagged.sum() * 8 < n - 16)   # dense / sparse form
        if self.cover:
            assert np.bincount(rows[from_src], minlength=n)[self.src.astype(I64)].all()
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
            assert min(who) < 64 or max(who) >= self.k - 64
        assert any(0 in who for who in self.special.values()) and any(self.k - 1 in who for who in self.special.values())

    def nonzero_rows(self, hops):
        """How many vertices the sources reach in exactly `hops` clean hops: the non-zero rows of the state after that hop."""
        rows, cols = (x.astype(I64) for x in self.a.pairs())
        cur = np.zeros(self.n, dtype=bool)
        cur[self.src.astype(I64)] = True
        for _ in range(hops):
            nxt = np.zeros(self.n, dtype=bool)
            nxt[cols[cur[rows]]] = True
            cur = nxt
        return int(cur.sum())

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


def Forced(ctx, **opts):
    return ctx.options(expand_mode=2, expand_xcd_min_mb=0, **opts)
