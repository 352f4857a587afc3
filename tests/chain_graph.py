"""The constructed graph of the expand chain's form decisions (test_gpu_chain_forms.py, test_chain_graph_cpu.py).

spgemm.hip expand_device decides hop by hop what form the frontier is in: the first-hop shortcuts, the hop at which the chain
leaves the sorted-CSR form (T * expand_bits_ratio > nnz), how (a push when T * 32 <= nnz, else a scatter whose state is lazily
zeroed when |F| * 8 < n), and whether the empty source rows are dropped on the way (k >= 128 and the live rows fit a narrower
row stride).  Every quantity in those rules is read off this graph on the host, before anything goes to the device.

The graph is layered, so one matrix serves every hop:

  filler   vertices nothing reaches; their out-edges set nnz without changing any T
  L0       the source layer: live vertices (d0 out-edges into L1), vertices without out-edges, vertices whose every out-edge
           is tombstoned by dm (dirty graphs) and vertices that only reach dead ends of L1 (their rows die at hop 2)
  L1, L2   d1 / d2 out-edges into the next layer each; L1 also holds the dead ends
  L3       the last layer, and a few vertices that only dp reaches
  pad      isolated vertices that set n

T_h is counted per frontier entry (as oracle.delta_lmxm's flops are) over the BASE matrix, which is what mxm_flops and the first
hop's copy sum for the decision; the reported flops add the dp products and come from the oracle.
"""
import numpy as np

import oracle

U64, I64 = np.uint64, np.int64
SKIP = np.uint64(2**64 - 1)
LDS_LIMIT = 160 * 1024                       # gfx950: sharedMemPerBlock, what fgpu_init puts into lds_limit
SPARSE_LDS = 32 * 1024 + 16 * 256 * 4        # bitexpand.hip BP_SPARSE_LDS
FH_MAX_ROWS = 4096                           # spgemm.hip: the first-hop shortcuts take fewer rows than this
SIZES = {"s0": 1024, "n1": 2048, "n2": 2048, "n3": 1024, "nf": 1500}
SMALL = {"s0": 256, "n1": 512, "n2": 512, "n3": 512, "nf": 600}
NOOUT, TOMB, DIE, DEAD1, X3 = 8, 64, 64, 64, 8


def bits_stride(rows):
    """spgemm.hip bits_stride = bitexpand.hip bp_layout: 64-bit words between two rows of the bit state."""
    w = max(1, (rows + 63) // 64)
    if w > 64:
        return (w + 63) // 64 * 64
    p = 1
    while p < w:
        p <<= 1
    return p


def forced(ctx, **opts):
    """The context's guard with exactly these options: the chain tests choose expand_mode themselves."""
    assert "expand_mode" in opts
    return ctx.options(**opts)


def live_pattern(k, nlive):
    """Which of the k rows are live: the first and the last row are empty, rows 64..127 (a whole bit word) from 512 rows on and
    rows 256..511 (a whole wavefront of cr_rank_kernel, which owns 4 rows a lane) from 1024 on, the rest alternating."""
    empty = np.zeros(k, dtype=bool)
    empty[0] = empty[k - 1] = True
    if k >= 512:
        empty[64:128] = True
    if k >= 1024:
        empty[256:512] = True
    free = np.flatnonzero(~empty)
    need = (k - nlive) - int(empty.sum())
    assert 0 <= need <= len(free), (k, nlive)
    order = np.concatenate([free[::2], free[1::2][::-1]])
    empty[order[:need]] = True
    assert int(empty.sum()) == k - nlive
    return ~empty


def label_ids(n):
    return np.nonzero((oracle.mix64(np.arange(n, dtype=U64)) % np.uint64(4)) != 0)[0]


def reference(src, layers, n, label=None):
    """F from the valid sources, oracle.delta_lmxm per hop, the label filter: (result, flops, [F_0 .. F_hops])."""
    src = np.asarray(src, dtype=U64)
    k = len(src)
    valid = src != SKIP
    f = oracle.build_csr(k, n, np.arange(k, dtype=U64)[valid], src[valid])
    flops, fr = 0, [f]
    for m, dp, dm in layers:
        f, fl = oracle.delta_lmxm(f, m, dp, dm)
        flops += fl
        fr.append(f)
    if label is not None:
        rows, cols = f.pairs()
        keep = np.isin(cols, label)
        f = oracle.build_csr(k, n, rows[keep], cols[keep])
    return f, flops, fr


class Graph:
    def __init__(self, name, k, nlive, d, kinds, dirty=False, sizes=SIZES, nnz=None, n=None):
        """k rows of which `nlive` stay live to the end; the empty rows take `kinds` in turn ("skip": UINT64_MAX, "noout": a
        source without out-edges, "tomb": every out-edge tombstoned, "die2": live after the first hop, empty after the second).
        nnz(T) and n(F) are rules over the traversed edges and the frontier sizes of the clean-or-dirty chain: the filler and
        the padding make them hold exactly."""
        assert dirty or "tomb" not in kinds
        self.name, self.k, self.d, self.dirty, self.kinds = name, k, d, dirty, kinds
        s0, n1, n2, n3, nf = (sizes[x] for x in ("s0", "n1", "n2", "n3", "nf"))
        d0, d1, d2 = d
        assert d0 <= DEAD1 and d1 <= n2 and d2 <= n3
        self.L0 = L0 = nf
        noout0 = L0 + s0
        tomb0 = noout0 + NOOUT
        die0 = tomb0 + TOMB
        self.L1 = L1 = die0 + DIE
        dead0 = L1 + n1
        self.L2 = L2 = dead0 + DEAD1
        self.L3 = L3 = L2 + n2
        x30 = L3 + n3
        self.nbase = nbase = x30 + X3
        # ---- the rows
        live = self.live = live_pattern(k, nlive)
        src = np.full(k, SKIP, dtype=U64)
        lr = np.flatnonzero(live)
        src[lr] = (L0 + np.arange(len(lr)) % s0).astype(U64)
        assert len(lr) >= 2
        src[lr[1]] = src[lr[0]]                                  # two rows with the same source, both live
        er = np.flatnonzero(~live)
        self.kind_of = {}
        for j, i in enumerate(er.tolist()):
            kd = kinds[j % len(kinds)]
            q = j // len(kinds)
            self.kind_of[i] = kd
            if kd == "noout":
                src[i] = noout0 + q % NOOUT
            elif kd == "tomb":
                src[i] = tomb0 + q % TOMB
            elif kd == "die2":
                src[i] = die0 + q % DIE
            else:
                assert kd == "skip"
        self.src = src
        # ---- the edges of the layers
        e = []

        def fan(first, count, deg, to, width, shift=0):
            a = np.repeat(np.arange(count, dtype=I64), deg)
            t = np.tile(np.arange(deg, dtype=I64), count)
            e.append((first + a, to + (a * deg + t + shift) % width))

        fan(L0, s0, d0, L1, n1)
        fan(tomb0, TOMB, d0, L1, n1, 7)
        fan(die0, DIE, d0, dead0, DEAD1)
        fan(L1, n1, d1, L2, n2)
        fan(L2, n2, d2, L3, n3)
        rows = np.concatenate([x[0] for x in e])
        cols = np.concatenate([x[1] for x in e])
        core = len(rows)
        assert len(set(zip(rows.tolist(), cols.tolist()))) == core
        # ---- the delta layers: every tombstoned row of L0, and a few entries at every layer
        if dirty:
            ta = np.repeat(np.arange(TOMB, dtype=I64), d0)
            tt = np.tile(np.arange(d0, dtype=I64), TOMB)
            a1 = np.arange(3, n1, 97, dtype=I64)
            a2 = np.arange(5, n2, 89, dtype=I64)
            dmr = np.concatenate([tomb0 + ta, L1 + a1, L2 + a2])
            dmc = np.concatenate([L1 + (ta * d0 + tt + 7) % n1, L2 + (a1 * d1) % n2, L3 + (a2 * d2 + 1) % n3])
            b0 = np.arange(2, s0, 61, dtype=I64)
            b1 = np.arange(1, n1, 83, dtype=I64)
            b2 = np.arange(4, n2, 79, dtype=I64)
            dpr = np.concatenate([L0 + b0, L1 + b1, L2 + b2])
            dpc = np.concatenate([L1 + (b0 * d0 + d0 + 5) % n1, L2 + (b1 * d1 + d1 + 3) % n2, x30 + b2 % X3])

        def layers_for(nn, r, c):
            a = oracle.build_csr(nn, nn, r.astype(U64), c.astype(U64))
            if not dirty:
                return a, None, None
            return (a, oracle.build_csr(nn, nn, dpr.astype(U64), dpc.astype(U64)),
                    oracle.build_csr(nn, nn, dmr.astype(U64), dmc.astype(U64)))

        # ---- T and |F| from the core graph (the filler is not reached, the padding has no edges), then nnz and n by their rules
        a, dp, dm = layers_for(nbase, rows, cols)
        if dirty:
            assert a.has_edges(dmr, dmc).all() and not a.has_edges(dpr, dpc).any()
        _, _, fr = reference(src, [(a, dp, dm)] * 3, nbase)
        deg = np.diff(a.rowptr.astype(I64))
        T = [int(deg[f.colidx.astype(I64)].sum()) for f in fr[:3]]
        F = [f.nnz for f in fr]
        self.nnz = int(nnz(T)) if callable(nnz) else int(nnz)
        self.n = int(n(F)) if callable(n) else int(n if n is not None else nbase + 9)
        assert self.n >= nbase and self.nnz >= core, (name, self.n, nbase, self.nnz, core)
        fill = self.nnz - core
        per, extra = divmod(fill, nf)
        assert per + 1 <= nbase - nf
        cnt = np.full(nf, per, dtype=I64)
        cnt[:extra] += 1
        fr_ = np.repeat(np.arange(nf, dtype=I64), cnt)
        ft = np.concatenate([np.arange(c, dtype=I64) for c in cnt.tolist()]) if fill else np.zeros(0, dtype=I64)
        fc = nf + (fr_ * 131 + ft) % (nbase - nf)               # into every layer: rows of A' of mixed lengths, none into the filler
        self.a, self.dp, self.dm = layers_for(self.n, np.concatenate([rows, fr_]), np.concatenate([cols, fc]))
        self.check_shape(T, F)

    # ---- what the graph holds, from the graph itself -------------------------------------------------------------------
    def layers(self, hops):
        return [(self.a, self.dp, self.dm)] * hops

    def ref(self, hops, label=False, src=None, layers=None):
        """(result, flops, checksum, [F_0 .. F_hops]) of the oracle, computed once for the graph's own layers and shared."""
        key = (hops, label, None if src is None else src.tobytes())
        if not hasattr(self, "_refs"):
            self._refs = {}
        if layers is not None or key not in self._refs:
            c, flops, fr = reference(self.src if src is None else src, layers or self.layers(hops), self.n,
                                     label_ids(self.n) if label else None)
            if layers is not None:
                return c, flops, oracle.checksum(c), fr
            self._refs[key] = (c, flops, oracle.checksum(c), fr)
        return self._refs[key]

    def label(self):
        return oracle.bits_from_ids(self.n, label_ids(self.n))

    def frontiers(self):
        """F_0 .. F_3, T_0 .. T_2 over the base matrix, and the rows that are non-empty after each hop."""
        if not hasattr(self, "_fr"):
            fr = self.ref(3)[3]
            deg = np.diff(self.a.rowptr.astype(I64))
            T = [int(deg[f.colidx.astype(I64)].sum()) for f in fr[:3]]
            live = [np.diff(f.rowptr.astype(I64)) > 0 for f in fr]
            self._fr = (fr, T, live)
        return self._fr

    def check_shape(self, T0, F0):
        a, n, k = self.a, self.n, self.k
        fr, T, live = self.frontiers()
        assert a.nnz == self.nnz and a.nrows == n and T == T0 and [f.nnz for f in fr] == F0
        rows, cols = (x.astype(I64) for x in a.pairs())
        assert not (cols < self.L0).any()                         # nothing reaches the filler: its out-edges change no T
        assert (np.diff(a.rowptr.astype(I64))[self.nbase:] == 0).all()
        # the rows that are empty after each hop, by kind
        kind = np.array([self.kind_of.get(i, "live") for i in range(k)])
        assert np.array_equal(live[0], kind != "skip")
        assert np.array_equal(live[1], (kind == "live") | (kind == "die2"))
        assert np.array_equal(live[2], kind == "live") and np.array_equal(live[3], kind == "live")
        assert np.array_equal(kind == "live", self.live)
        for kd in self.kinds:
            assert (kind == kd).any(), kd
        # placement: the first and the last row, a whole bit word, a whole wavefront of cr_rank_kernel, alternating rows
        dead = ~self.live
        assert dead[0] and dead[k - 1]
        assert k < 512 or dead[64:128].all()
        assert k < 1024 or dead[256:512].all()
        alt = dead[:-2] & ~dead[1:-1] & dead[2:]
        assert alt.any()
        lr = np.flatnonzero(self.live)
        assert self.src[lr[0]] == self.src[lr[1]]
        if self.dirty:
            clean = reference(self.src, [(self.a, None, None)] * 3, n)[0]
            assert not (clean == self.ref(3)[0])                  # the delta layers change the result
        lab = self.ref(3, label=True)[0]
        assert 0 < lab.nnz < self.ref(3)[0].nnz                   # so does the label

    # ---- a cell: every inequality it names ------------------------------------------------------------------------------
    def check_cell(self, hops, mode=0, ratio=28, first_hop=1, compact_opt=1, hyper=None, leave=None, how=None, zero=None,
                   compact=False, pulls=()):
        """Asserts, from the host graph, that a `hops`-hop chain under these options leaves the CSR form at hop index `leave`
        (None: never) by `how` ("push" / "scatter"), the scatter's state zeroed `zero` ("lazy" / "full"), the empty rows dropped
        or not (`compact`), and the pulls that follow in the forms `pulls` ("sparse" / "dense", one per pulled hop)."""
        fr, T, live = self.frontiers()
        n, nnz, k = self.n, self.nnz, self.k
        shortcut = mode != 2 and first_hop and 0 < k < FH_MAX_ROWS and fr[0].nnz > 0
        left = None
        for h in range(hops):
            if (h == 0 and shortcut) or mode == 1 or h == hyper or fr[h].nnz == 0:
                continue
            if mode == 0:
                if leave is None or h < leave:
                    assert T[h] * ratio <= nnz, (self.name, h, T[h], ratio, nnz)
                    continue
                assert h == leave and T[h] * ratio > nnz, (self.name, h, T[h], ratio, nnz)
            left = h
            break
        assert left == leave, (self.name, left, leave)
        if leave is None:
            assert how is None and zero is None and not compact and not pulls
            return
        nl = int(live[leave].sum())
        applies = bool(compact_opt) and k >= 128 and nl > 0 and bits_stride(nl) < bits_stride(k)
        assert applies == compact, (self.name, k, nl, bits_stride(nl), bits_stride(k))
        w = ((nl if compact else k) + 63) // 64
        if how == "push":
            assert T[leave] * 32 <= nnz and zero is None, (self.name, T[leave], nnz)
        else:
            assert how == "scatter" and T[leave] * 32 > nnz, (self.name, T[leave], nnz)
            fits = w * 2048 + SPARSE_LDS <= LDS_LIMIT
            if zero == "lazy":
                assert fr[leave].nnz * 8 < n and fits, (self.name, fr[leave].nnz, n, w)
            else:
                assert zero == "full" and (fr[leave].nnz * 8 >= n or not fits), (self.name, fr[leave].nnz, n, w)
        got = []
        for h in range(leave + (how == "push"), hops):
            if h == leave:
                rows_in = min(fr[h].nnz, n)                       # bp_from_csr: an upper bound is the state's row count
            else:
                rows_in = len(np.unique(fr[h].colidx))
                # (a row that a tombstone of the hop before emptied may still be flagged: the device's count is within those of this)
                assert abs(rows_in * 8 - n) > 8 * self.tombstones_from(fr[h - 1]), (self.name, h, rows_in, n)
            got.append("sparse" if rows_in * 8 < n else "dense")
        assert tuple(pulls) == tuple(got), (self.name, pulls, got)

    def tombstones_from(self, f):
        if self.dm is None:
            return 0
        reached = np.zeros(self.n, dtype=bool)
        reached[f.colidx.astype(I64)] = True
        return int(reached[self.dm.pairs()[0].astype(I64)].sum())

    def count_pull(self, hops, leave, compact, checksum):
        """The form of the fused counting pull of a chain that left at `leave` < hops - 1 or by scatter at hops - 1."""
        fr, _, live = self.frontiers()
        h = hops - 1
        rows_in = min(fr[h].nnz, self.n) if h == leave else len(np.unique(fr[h].colidx))
        w = ((int(live[leave].sum()) if compact else self.k) + 63) // 64
        fits = (w * 2048 if checksum else 0) + SPARSE_LDS <= LDS_LIMIT
        return "sparse" if rows_in * 8 < self.n and fits else "dense"

    def figures(self):
        fr, T, live = self.frontiers()
        return {"T": T, "F": [f.nnz for f in fr], "nnz": self.nnz, "n": self.n, "k": self.k,
                "nlive": [int(x.sum()) for x in live]}

    def as_built(self):
        f = self.figures()
        return (f["k"], tuple(f["nlive"][:3]), tuple(f["T"]), f["F"][1], f["F"][2], f["nnz"], f["n"])

    # ---- on the device ---------------------------------------------------------------------------------------------------
    def device(self, ctx):
        if not hasattr(self, "_dev"):
            coo = lambda m: ctx.mat_from_coo(m.nrows, m.ncols, *m.pairs()) if m is not None else None
            self._dev = tuple(coo(m) for m in (self.a, self.dp, self.dm))
        return self._dev

    def device_layers(self, ctx, hops):
        a, dp, dm = self.device(ctx)
        return ([a] * hops, [dp] * hops, [dm] * hops) if self.dirty else ([a] * hops, None, None)

    def free(self):
        for m in getattr(self, "_dev", ()):
            if m is not None:
                m.free()
        self.__dict__.pop("_dev", None)


# ---- the graphs ------------------------------------------------------------------------------------------------------------
# std: T grows 10x a hop and nnz == 32 * T1, so integer ratios separate the cells and the hop-1 entry sits on the push side of
# its bar; std-1 has one edge less (the scatter side); n == 8 |F1| + 1 is the lazy side of the scatter's zeroing, std-full
# (n == 8 |F1|) the other.  A third of the empty rows die at hop 2: a chain that leaves at hop index 1 keeps every row
# (675 live of 1024: 16 words either way), one that leaves at hop index 2 drops them (500 live: 8 words).
BOUNDARIES = [(127, 60), (128, 64), (128, 65), (1024, 512), (1024, 513), (4095, 2048), (4096, 2048), (8192, 4096), (8192, 4097)]
_STD = dict(k=1024, nlive=500, d=(2, 10, 10), kinds=("skip", "noout", "die2"))
SPECS = {
    "std": dict(_STD, nnz=lambda T: 32 * T[1], n=lambda F: 8 * F[1] + 1),
    "std-1": dict(_STD, nnz=lambda T: 32 * T[1] - 1, n=lambda F: 8 * F[1] + 1),
    "std-full": dict(_STD, nnz=lambda T: 32 * T[1] - 1, n=lambda F: 8 * F[1]),
    "std-dirty": dict(_STD, kinds=("skip", "noout", "tomb", "die2"), dirty=True, nnz=lambda T: 32 * T[1],
                      n=lambda F: 8 * F[1] + 1),
    # a frontier that is still light at hop index 2: the scatter there is lazily zeroed
    "thin": dict(k=300, nlive=150, d=(1, 6, 10), kinds=("skip", "noout", "die2"), nnz=100000, n=9001),
    # a first hop too heavy to be pushed; only UINT64_MAX rows are empty, which is all a chain that leaves at hop 0 can drop
    "heavy0": dict(k=1024, nlive=500, d=(8, 10, 10), kinds=("skip",), nnz=100000, n=9001),
    # n < 4096: the emission is the ballot transpose whatever expand_emit_sort says
    "small": dict(k=200, nlive=90, d=(2, 6, 6), kinds=("skip", "noout", "tomb", "die2"), dirty=True, sizes=SMALL,
                  nnz=lambda T: 32 * T[1], n=3001),
}
for _k, _nl in BOUNDARIES:
    # two hops over dirty layers, every kind of empty row that a chain leaving at hop index 1 can drop
    SPECS["cb-%d-%d" % (_k, _nl)] = dict(k=_k, nlive=_nl, d=(1, 10, 10), kinds=("skip", "noout", "tomb"), dirty=True,
                                         nnz=lambda T: max(20 * T[1], 60000), n=9001)

# The figures of every graph as built (test_chain_graph_cpu.py holds the graphs to them): name: (k, live rows after hop 0 / 1 / 2,
# T0 / T1 / T2 over the base matrix, |F1|, |F2|, nnz, n).  With a cell's ratio these re-derive every inequality of its path by hand.
FIGURES = {
    "std": (1024, (849, 674, 500), (1348, 10000, 100000), 1348, 10000, 320000, 10785),
    "std-1": (1024, (849, 674, 500), (1348, 10000, 100000), 1348, 10000, 319999, 10785),
    "std-full": (1024, (849, 674, 500), (1348, 10000, 100000), 1348, 10000, 319999, 10784),
    "std-dirty": (1024, (893, 631, 500), (1524, 10090, 100890), 1271, 10089, 322880, 10169),
    "thin": (300, (250, 200, 150), (200, 900, 9000), 200, 900, 100000, 9001),
    "heavy0": (1024, (500, 500, 500), (4000, 40000, 400000), 4000, 40000, 100000, 9001),
    "small": (200, (172, 117, 90), (288, 1092, 6564), 236, 1094, 34944, 3001),
    "cb-127-60": (127, (104, 60, 60), (82, 610, 6090), 61, 609, 60000, 9001),
    "cb-128-64": (128, (106, 64, 64), (85, 660, 6590), 66, 659, 60000, 9001),
    "cb-128-65": (128, (107, 65, 65), (86, 670, 6690), 67, 669, 60000, 9001),
    "cb-1024-512": (1024, (853, 512, 512), (682, 5210, 52100), 521, 5210, 104200, 9001),
    "cb-1024-513": (1024, (853, 513, 513), (683, 5220, 52200), 522, 5220, 104400, 9001),
    "cb-4095-2048": (4095, (3412, 2048, 2048), (2730, 20820, 208230), 2082, 20823, 416400, 9001),
    "cb-4096-2048": (4096, (3413, 2048, 2048), (2730, 20820, 208230), 2082, 20823, 416400, 9001),
    "cb-8192-4096": (8192, (6826, 4096, 4096), (5461, 41640, 416470), 4164, 41647, 832800, 9001),
    "cb-8192-4097": (8192, (6827, 4097, 4097), (5462, 41650, 416570), 4165, 41657, 833000, 9001),
}

_made = {}


def graph(name):
    if name not in _made:
        _made[name] = Graph(name, **SPECS[name])
    return _made[name]


def leave_ratio(g, h):
    """The smallest ratio at which a chain over g leaves at hop index h (the hops before it stay: T grows 10x a hop)."""
    _, T, _ = g.frontiers()
    r = g.nnz // T[h] + 1
    assert 1 <= r <= 1024
    return r


# ---- the cells -------------------------------------------------------------------------------------------------------------
# id: (graph, hops, options, the path check_cell asserts).  The ratios are the ones the graphs' figures give (test_chain_graph_cpu.py
# re-derives every inequality): std has T = 1348, 10000, 100000 and nnz = 320000, so ratio 3 never leaves, 4..32 leave at hop
# index 2, 33..237 at hop index 1, and from 238 the general first hop leaves at hop 0.
def _path(leave=None, how=None, zero=None, compact=False, pulls=()):
    return dict(leave=leave, how=how, zero=zero, compact=compact, pulls=pulls)


CELLS = {
    # 1. never leaves
    "1 ratio too small": ("std", 3, dict(expand_mode=0, expand_bits_ratio=3), _path()),
    "1 mode 1": ("std", 3, dict(expand_mode=1, expand_bits_ratio=1024), _path()),
    # 2. leaves at hop index 1 / 2; both sides of T * ratio > nnz (std / std-1 at ratio 32) and of T * 32 <= nnz (at ratio 33)
    "2 T1 * ratio == nnz: stays, leaves at 2, full": ("std", 3, dict(expand_mode=0, expand_bits_ratio=32),
                                                      _path(2, "scatter", "full", True, ("dense",))),
    "2 T1 * ratio == nnz + 1: leaves at 1, lazy": ("std-1", 3, dict(expand_mode=0, expand_bits_ratio=32),
                                                   _path(1, "scatter", "lazy", False, ("sparse", "dense"))),
    "2 T1 * 32 == nnz: push at 1": ("std", 3, dict(expand_mode=0, expand_bits_ratio=33), _path(1, "push", None, False, ("dense",))),
    "2 T1 * 32 == nnz + 1: scatter at 1": ("std-1", 3, dict(expand_mode=0, expand_bits_ratio=33),
                                           _path(1, "scatter", "lazy", False, ("sparse", "dense"))),
    "2 |F1| * 8 == n: scatter at 1, full": ("std-full", 3, dict(expand_mode=0, expand_bits_ratio=32),
                                            _path(1, "scatter", "full", False, ("dense", "dense"))),
    "2 leaves at 2, full": ("std", 3, dict(expand_mode=0, expand_bits_ratio=8), _path(2, "scatter", "full", True, ("dense",))),
    "2 leaves at 2, lazy": ("thin", 3, dict(expand_mode=0, expand_bits_ratio=12), _path(2, "scatter", "lazy", True, ("sparse",))),
    "2 dirty, push at 1": ("std-dirty", 3, dict(expand_mode=0, expand_bits_ratio=33), _path(1, "push", None, False, ("dense",))),
    "2 dirty, leaves at 2": ("std-dirty", 3, dict(expand_mode=0, expand_bits_ratio=8), _path(2, "scatter", "full", True, ("dense",))),
    # 3. leaves at hop 0
    "3 mode 2, light first hop": ("std", 3, dict(expand_mode=2), _path(0, "push", None, False, ("sparse", "dense"))),
    "3 mode 2, heavy first hop": ("heavy0", 3, dict(expand_mode=2), _path(0, "scatter", "lazy", True, ("sparse", "dense", "dense"))),
    "3 mode 0, general first hop": ("std", 3, dict(expand_mode=0, expand_first_hop=0, expand_bits_ratio=238),
                                    _path(0, "push", None, False, ("sparse", "dense"))),
    # 4. T summed by mxm_flops instead of taken from the first hop's copy: the path of "2 T1 * 32 == nnz: push at 1"
    "4 T by mxm_flops": ("std", 3, dict(expand_mode=0, expand_first_hop=0, expand_bits_ratio=33), _path(1, "push", None, False, ("dense",))),
    # 5. a hypersparse base at hop index 1: the chain stays CSR over it and leaves one hop later
    "5 hypersparse at 1": ("std", 3, dict(expand_mode=0, expand_bits_ratio=33, hyper=1), _path(2, "scatter", "full", True, ("dense",))),
}
# 6. the (k, nlive) boundaries: two hops, leaving at hop index 1 at the ratio nnz // T1 + 1; whether the rows are dropped
BOUNDARY_COMPACTS = {(127, 60): False, (128, 64): True, (128, 65): False, (1024, 512): True, (1024, 513): False,
                     (4095, 2048): True, (4096, 2048): True, (8192, 4096): True, (8192, 4097): False}
BOUNDARY_RATIO = {(127, 60): 99, (128, 64): 91, (128, 65): 90}      # every other boundary graph has nnz == 20 * T1: ratio 21
for (_k, _nl), _c in BOUNDARY_COMPACTS.items():
    for _opt in (1, 0):
        _r = BOUNDARY_RATIO.get((_k, _nl), 21)
        if _k <= 128:
            _p = _path(1, "push", None, bool(_c and _opt), ())
        else:
            _p = _path(1, "scatter", "lazy" if _k == 1024 else "full", bool(_c and _opt), ("sparse" if _k == 1024 else "dense",))
        CELLS["6 k %d, live %d, compact %d" % (_k, _nl, _opt)] = (
            "cb-%d-%d" % (_k, _nl), 2, dict(expand_mode=0, expand_bits_ratio=_r, expand_compact=_opt), _p)
# 7. the ends run on these (the chain of a probe is one hop shorter: its cell is built for that length)
CELLS.update({
    "7 compacted, scatter at 1": ("cb-1024-512", 3, dict(expand_mode=0, expand_bits_ratio=21),
                                  _path(1, "scatter", "lazy", True, ("sparse", "dense"))),
    "7 small, compacted, push at 1": ("small", 3, dict(expand_mode=0, expand_bits_ratio=33), _path(1, "push", None, True, ("dense",))),
    "7 probe, push at 1": ("std", 2, dict(expand_mode=0, expand_bits_ratio=33), _path(1, "push", None, False, ())),
    "7 probe, compacted, scatter at 1": ("cb-1024-512", 2, dict(expand_mode=0, expand_bits_ratio=21),
                                         _path(1, "scatter", "lazy", True, ("sparse",))),
    "7 probe, small, compacted, push at 1": ("small", 2, dict(expand_mode=0, expand_bits_ratio=33), _path(1, "push", None, True, ())),
})


def check(cell):
    """The builder's self-checks for one cell: the graph's shape (on construction) and every inequality of its path."""
    name, hops, opts, path = CELLS[cell]
    g = graph(name)
    g.check_cell(hops, mode=opts["expand_mode"], ratio=opts.get("expand_bits_ratio", 28), first_hop=opts.get("expand_first_hop", 1),
                 compact_opt=opts.get("expand_compact", 1), hyper=opts.get("hyper"), **path)
    return g


def device_options(opts):
    return {k: v for k, v in opts.items() if k != "hyper"}
