"""GPU: the whole-frontier fgpu_expand_count classes its degree-one sources by their target (spgemm.hip scan_build_classes).

Over a clean hop 0, sources whose only out-edge over m[0] ends at the same target share one bit of a pass: a class of m sources
takes one row in the group of scale 2^k for every set bit k < kmax of m and m >> kmax rows in the top group, a pass holds rows
of one scale, and kmax in [0, 5] minimises the passes.  Every case below runs the 3-hop chain as whole-frontier calls of 64- or
128-row passes on one lane and on three and compares (nnz, checksum, flops) with the CPU oracle over all sources, (nnz, flops)
with the same sources sent as calls of 1024 rows below `expand_scan_min`, the number of passes with a numpy model of the plan,
and the profile's "scan classes" record with whether hop 0 was clean."""
import collections
import ctypes as C

import numpy as np
import pytest

import oracle
from falkordb_amd import engine

pytestmark = pytest.mark.gpu

U64 = np.uint64
NONE = np.iinfo(np.uint64).max
N = 1 << 13
FANS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 119)
SCOPE = "scan classes"
Plan = collections.namedtuple("Plan", "nlive passes kmax groups names")


def csr_of(n, rows, cols):
    """the CSR of the DISTINCT (row, col) pairs, and those pairs"""
    key = np.unique((np.asarray(rows, dtype=U64) << U64(32)) | np.asarray(cols, dtype=U64))
    r, c = key >> U64(32), key & U64(0xFFFFFFFF)
    return oracle.build_csr(n, n, r, c), r, c


class Graph:
    """Vertex layout: the fan targets first, then the members of every fan (one out-edge, to the fan's target), then `share`
    vertices of out-degree 2 and 3 with one edge into a fan target, then `dead` vertices without out-edges; every other vertex
    (the targets too) has `lo` .. `hi` random out-edges."""

    def __init__(self, ctx, fans, n=N, share=0, dead=0, lo=2, hi=8, seed=1):
        rng = np.random.default_rng(0x5CA9 + seed)
        nf = len(fans)
        self.targets = np.arange(nf, dtype=U64)
        first = nf + np.concatenate([[0], np.cumsum(fans)]).astype(np.int64)
        self.members = [np.arange(first[j], first[j + 1], dtype=U64) for j in range(nf)]
        v = int(first[-1])
        self.sharers = np.arange(v, v + share, dtype=U64)
        self.dead = np.arange(v + share, v + share + dead, dtype=U64)
        assert v + share + dead < n
        rows = [np.concatenate(self.members)]                     # member -> its target
        cols = [np.repeat(self.targets, fans).astype(U64)]
        for i, s in enumerate(self.sharers):                      # a fan target, and one or two other vertices
            k = 1 + i % 2
            rows.append(np.full(1 + k, s, dtype=U64))
            cols.append(np.concatenate([[self.targets[i % nf]], rng.choice(np.arange(nf, n), k, replace=False)]).astype(U64))
        plain = np.concatenate([self.targets, np.arange(v + share + dead, n, dtype=U64)])
        # k columns s0 + i * stride (mod n, a power of two; stride odd): distinct, so the degree is the k that was drawn
        k = rng.integers(lo, hi + 1, len(plain))
        i = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
        s0, stride = rng.integers(0, n, len(plain)), 2 * rng.integers(0, n // 2, len(plain)) + 1
        rows.append(np.repeat(plain, k))
        cols.append(((np.repeat(s0, k) + i * np.repeat(stride, k)) % n).astype(U64))
        self.plain = plain[nf:]
        self.n = n
        self.a, r, c = csr_of(n, np.concatenate(rows), np.concatenate(cols))
        self.ctx = ctx
        self.A = ctx.mat_from_coo(n, n, r, c)
        self.mats = [self.A]

    def delta(self, pairs_plus, pairs_minus):
        """(dp, dm) on the device and on the host; dp must lie outside the matrix and dm inside it"""
        out = []
        for pairs in (pairs_plus, pairs_minus):
            h, r, c = csr_of(self.n, [p[0] for p in pairs], [p[1] for p in pairs])
            d = self.ctx.mat_from_coo(self.n, self.n, r, c)
            self.mats.append(d)
            out.append((d, h))
        return out

    def has(self, r, c):
        b, e = int(self.a.rowptr[int(r)]), int(self.a.rowptr[int(r) + 1])
        return int(c) in self.a.colidx[b:e]

    def random_delta(self, seed, k=40):
        rng = np.random.default_rng(seed)
        plus = [(r, c) for r, c in zip(rng.integers(0, self.n, 3 * k), rng.integers(0, self.n, 3 * k)) if not self.has(r, c)][:k]
        e = rng.choice(self.a.nnz, k, replace=False)
        rows = np.repeat(np.arange(self.n), np.diff(self.a.rowptr.astype(np.int64)))
        return self.delta(plus, [(rows[i], self.a.colidx[i]) for i in e])

    def free(self):
        for m in self.mats:
            m.free()


def plan(a, src, rows, classed=True):
    """The numpy model of the pass plan: (live rows, passes, kmax, rows per group)."""
    src = np.asarray(src, dtype=U64)
    ok = src != NONE
    rp = a.rowptr.astype(np.int64)
    deg = np.zeros(len(src), dtype=np.int64)
    deg[ok] = rp[src[ok].astype(np.int64) + 1] - rp[src[ok].astype(np.int64)]
    live = np.nonzero(deg > 0)[0]
    nlive = len(live)
    if not classed:
        return nlive, -(-nlive // rows), 0, [nlive]
    one = live[deg[live] == 1]
    m = np.unique(a.colidx[rp[src[one].astype(np.int64)]], return_counts=True)[1].astype(np.int64)
    best = None
    for kmax in range(6):
        g = [int(((m >> k) & 1).sum()) if k < kmax else int((m >> k).sum()) for k in range(kmax + 1)]
        g[0] += nlive - len(one)
        p = sum(-(-r // rows) for r in g)
        if best is None or p < best[0]:
            best = (p, kmax, g)
    return (nlive,) + best


def count(ctx, src, m, dp=None, dm=None, label=None, want_checksum=True, want_flops=True):
    """engine.expand_count with a flops pointer that can be left out"""
    src = engine._u64(src)
    lab = engine._u64(label) if label is not None else None
    nnz, cs, flops = C.c_uint64(), C.c_uint64(), C.c_uint64()
    engine.check(ctx.lib.fgpu_expand_count(ctx._h, engine._p(src), len(src), engine._hop_arrays(m),
                                           engine._hop_arrays(dp) if dp is not None else None,
                                           engine._hop_arrays(dm) if dm is not None else None, len(m), engine._p(lab), C.byref(nnz),
                                           C.byref(cs) if want_checksum else None, C.byref(flops) if want_flops else None))
    return nnz.value, cs.value, flops.value


def reference(src, layers, label=None):
    """(nnz, checksum, flops) of the oracle over all sources, every row hashed by its index in `src`"""
    if label is None and not (src == NONE).any():
        return tuple(oracle.expand_summary_omp(src, layers, chunk=512, threads=8)[:3])
    # expand_summary_omp takes neither an empty row nor a label: its own steps, with the empty rows of the call left empty in F
    live = np.nonzero(src != NONE)[0]
    c = oracle.build_csr(len(src), layers[0][0].nrows, live.astype(U64), src[live])
    flops = 0
    for m, dp, dm in layers:
        c, fl = oracle.delta_lmxm_omp(c, m, dp, dm, 8)
        flops += fl
    if label is None:
        return c.nnz, oracle.checksum_omp(c, 8), flops
    keep = label[c.colidx.astype(np.int64)]
    rows = np.repeat(np.arange(c.nrows), np.diff(c.rowptr).astype(np.int64))[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=c.nrows))]).astype(U64)
    cl = oracle.CSR(c.nrows, c.ncols, rp, c.colidx[keep])
    return cl.nnz, oracle.checksum_omp(cl, 8), flops


def check(ctx, g, src, rows, dp=None, dm=None, label=None, want_checksum=True, want_flops=True, modes=(0, 2), **opts):
    """One case: the whole-frontier call in every (lanes, mode) against the oracle, the 1024-row calls and the plan's model.
    dp / dm: per hop, None or a (device, host) pair.  Returns the model's plan and the last call's profile names."""
    hops = 3
    dp = dp or [None] * hops
    dm = dm or [None] * hops
    dev = lambda x: [p[0] if p else None for p in x]
    host = lambda x, h: x[h][1] if x[h] else None
    layers = [(g.a, host(dp, h), host(dm, h)) for h in range(hops)]
    kw = dict(dp=dev(dp), dm=dev(dm), label=oracle.bits_from_ids(g.n, np.nonzero(label)[0]) if label is not None else None)
    ref = reference(src, layers, label)
    want = (ref[0], ref[1] if want_checksum else 0, ref[2] if want_flops else 0)
    clean0 = all(x is None or x[1].nnz == 0 for x in (dp[0], dm[0]))
    # a dirty hop 0: live = an entry in m[0] or dp[0]; the model counts the rows of m[0], so such cases keep dp[0] on live rows
    nlive, passes, kmax, groups = plan(g.a, src, rows, classed=clean0)
    # ... the same sources as calls of 1024 rows, below expand_scan_min: nnz and flops add up (a checksum hashes call rows)
    bn = bf = 0
    for c0 in range(0, len(src), 1024):
        r = count(ctx, src[c0:c0 + 1024], [g.A] * hops, **kw)
        bn, bf = bn + r[0], bf + r[2]
    assert (bn, bf) == (ref[0], ref[2])
    for lanes, mode in [(1, m) for m in modes] + [(3, m) for m in modes]:
        with ctx.options(expand_scan_min=1, expand_scan_rows=rows, expand_scan_lanes=lanes, expand_mode=mode, **opts):
            ctx.prof_enable(True)
            try:
                got = count(ctx, src, [g.A] * hops, want_checksum=want_checksum, want_flops=want_flops, **kw)
                names = [p["kernel"] for p in ctx.prof_read()]
            finally:
                ctx.prof_enable(False)
            print(f"lanes {lanes} mode {mode}: got {got} want {want} passes {ctx.get_option('expand_scan_last_passes')} "
                  f"model {passes} kmax {kmax} groups {groups}")
            assert got == want, (lanes, mode, got, want)
            assert ctx.get_option("expand_scan_last_live") == nlive
            assert ctx.get_option("expand_scan_last_passes") == passes, (lanes, mode, kmax, groups)
            assert (SCOPE in names) == clean0, names
    return Plan(nlive, passes, kmax, groups, names)


def mixed_sources(g, rng, nplain=150, nulls=9):
    """every fan member, sharer, dead vertex and fan target, `nplain` plain vertices and `nulls` empty rows, shuffled"""
    src = np.concatenate(g.members + [g.sharers, g.dead, g.targets, rng.choice(g.plain, nplain, replace=False),
                                      np.full(nulls, NONE, dtype=U64)]).astype(U64)
    rng.shuffle(src)
    return src


@pytest.fixture(scope="module")
def fans(ctx):
    g = Graph(ctx, FANS, share=40, dead=25)
    yield g
    g.free()


@pytest.mark.parametrize("rows", [64, 128])
def test_fans_of_every_size_among_other_sources(ctx, fans, rows):
    """Fans of 1 .. 119 members on distinct targets, among sources of degree 2 and 3 that share those targets, sources without
    out-edges, empty rows, plain sources and the fan targets themselves (sources of the scan too)."""
    src = mixed_sources(fans, np.random.default_rng(rows))
    nlive, passes, kmax, groups, names = check(ctx, fans, src, rows)
    assert kmax >= 1 and passes < -(-nlive // rows) and len(src) - nlive >= 25 + 9


@pytest.mark.parametrize("nf", [64, 65])
def test_a_group_of_exactly_one_pass_and_of_one_row_more(ctx, nf):
    """nf fans of four members and nf plain sources at 64-row passes: kmax = 2 with nf rows in group 0, none in group 1 and nf
    in the top group — one full pass each at 64, a full pass and a one-row pass each at 65."""
    g = Graph(ctx, (4,) * nf, seed=nf)
    try:
        rng = np.random.default_rng(nf)
        src = np.concatenate(g.members + [rng.choice(g.plain, nf, replace=False)]).astype(U64)
        rng.shuffle(src)
        nlive, passes, kmax, groups, names = check(ctx, g, src, 64)
        assert (kmax, groups) == (2, [nf, 0, nf]) and passes == (2 if nf == 64 else 4)
    finally:
        g.free()


def test_every_source_in_one_fan_of_5000(ctx):
    """m = 5000 = 156 * 32 + 8: kmax = 5, 156 rows of scale 32 (two passes of 128) and one row of scale 8."""
    g = Graph(ctx, (5000,), seed=5)
    try:
        nlive, passes, kmax, groups, names = check(ctx, g, g.members[0], 128)
        assert (nlive, passes, kmax, groups) == (5000, 3, 5, [0, 0, 0, 1, 0, 156])
    finally:
        g.free()


def test_no_degree_one_source_keeps_the_plain_passes(ctx, fans):
    g = fans
    src = np.concatenate([g.sharers, g.targets, np.random.default_rng(3).choice(g.plain, 300, replace=False)]).astype(U64)
    nlive, passes, kmax, groups, names = check(ctx, g, src, 64)
    assert kmax == 0 and passes == -(-nlive // 64) and nlive == len(src)


@pytest.mark.parametrize("which", ["dm", "dp"])
def test_a_dirty_hop_0_is_not_classed(ctx, fans, which):
    """One tombstone on a fan member's only edge, or one added edge on a degree-one source: the rows of m[0] no longer say what
    a source reaches, every row keeps scale 1 and the call runs the plain passes."""
    g = fans
    member, target = g.members[5][2], g.targets[5]
    other = next(int(c) for c in range(100, g.n) if not g.has(member, c))
    dp, dm = g.delta([(member, other)] if which == "dp" else [], [(member, target)] if which == "dm" else [])
    src = mixed_sources(g, np.random.default_rng(11))
    empty = [None, None]
    nlive, passes, kmax, groups, names = check(ctx, g, src, 64, dp=[dp if which == "dp" else None] + empty,
                                        dm=[dm if which == "dm" else None] + empty)
    assert kmax == 0 and passes == -(-nlive // 64)


def test_dirty_hops_1_and_2_over_a_clean_hop_0_are_classed(ctx, fans):
    g = fans
    dp, dm = g.random_delta(77)
    src = mixed_sources(g, np.random.default_rng(12))
    nlive, passes, kmax, groups, names = check(ctx, g, src, 64, dp=[None, dp, dp], dm=[None, dm, dm])
    assert kmax >= 1


def test_a_destination_label(ctx, fans):
    g = fans
    label = oracle.mix64(np.arange(g.n, dtype=U64)) % U64(3) != 0
    nlive, passes, kmax, groups, names = check(ctx, g, mixed_sources(g, np.random.default_rng(13)), 128, label=label)
    assert kmax >= 1


def test_count_only(ctx, fans):
    nlive, passes, kmax, groups, names = check(ctx, fans, mixed_sources(fans, np.random.default_rng(14)), 64, want_checksum=False)
    assert kmax >= 1


def test_without_flops(ctx, fans):
    nlive, passes, kmax, groups, names = check(ctx, fans, mixed_sources(fans, np.random.default_rng(15)), 64, want_flops=False)
    assert kmax >= 1


def test_passes_that_end_in_csr_form_hash_their_classes(ctx):
    """Out-degrees of 1 and 2 on 2^15 vertices, and a bar no hop of a 64-row pass reaches (expand_bits_ratio = 1: T > nnz): every
    pass stays on the sorted-CSR products and count_csr_result hashes its rows with the classes' sums."""
    g = Graph(ctx, FANS, n=1 << 15, share=40, dead=25, lo=1, hi=2, seed=9)
    try:
        src = mixed_sources(g, np.random.default_rng(16), nplain=400)
        nlive, passes, kmax, groups, names = check(ctx, g, src, 64, modes=(0,), expand_bits_ratio=1)
        assert kmax >= 1
        assert not [k for k in names if k.startswith(("bp_", "xp_", "bit-state"))], names
    finally:
        g.free()
