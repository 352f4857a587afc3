"""A host model of the blocked pull layout (falkordb_amd/csrc/blocked.hip, blocked_build) and the graphs that walk it.

Plain numpy.  plan() restates how blocked_build sizes the windows and splits a window's tiles among workgroups,
padded_entries() how many 32-bit entries the builders store, and make_case() builds the three ragged graphs of
tests/test_gpu_blocked.py, block by block, so that every path of blocked_mxv_kernel and of the bk_* builders that the R-MAT
tests never take is taken: a second unit per workgroup, empty blocks at the start / in the middle / at the end of a unit's
tile range, units with nothing to do, windows shared by several workgroups on ragged shapes, the output-word field at 4095,
one-entry blocks, blocks of exactly 256 and of 257 entries, quads that mix rows r and r + 32, and hub rows whose 64-entry
chunks interleave in one bucket.  check_preconditions() asserts, for a case and a CU count, that the generator still reaches
each of them; tests/test_blocked_layout_cpu.py runs it without a GPU and the GPU tests run it before they launch anything.

One branch stays out of reach: the ragged end of x in load_block (gi < x_words32 < gi + 4).  fgpu_vxm and fgpu_bench_spmv
pad x to a multiple of 4096 bits, so x_words32 is a multiple of 128 and no 4-word load straddles its end; the C ABI has no
other way in, and none is added for it.

Names: M is the matrix being streamed (the `At` argument of engine.vxm(..., 3)), n x n; window w = rows [w << wbits,
(w + 1) << wbits); tile c = columns [c << 18, (c + 1) << 18); block (w, c); bucket (w, c, row & 31)."""
import functools

import numpy as np

import oracle

TILE_BITS = 18
TILE = 1 << TILE_BITS
CHUNK = 256          # entries per wavefront trip: a block is padded to a multiple of it
MAX_WBITS = 17
U64 = np.uint64

CASES = {"ragged4": 3 * TILE + 777, "split5": 5 * TILE - 100, "wide17": 257 * 65536 + 33}

# (wbits, nwindows, ntiles, nsplit, tiles_per) the issue's table gives at 256 CUs, and the same rules at 304
EXPECTED_PLAN = {
    ("ragged4", 256): (12, 193, 4, 4, 1), ("ragged4", 304): (12, 193, 4, 4, 1),
    ("split5", 256): (13, 160, 5, 4, 2), ("split5", 304): (13, 160, 5, 4, 2),
    ("wide17", 256): (17, 129, 65, 4, 17), ("wide17", 304): (17, 129, 65, 8, 9),
}

# windows whose non-empty tiles are exactly the listed ones (40 entries each)
HOLE_WINDOWS = {
    "ragged4": {30: [3], 31: [0]},
    # parts of 2 tiles: [0, 2) [2, 4) [4, 5) and one past ntiles
    "split5": {30: [1], 31: [2], 32: [4], 33: [0, 3]},
    # 256 CUs: parts of 17 tiles ([0, 17) .. [51, 65)); 304 CUs: parts of 9 ([0, 9) .. [54, 63) [63, 65))
    "wide17": {30: [64], 31: [0], 32: [51, 64], 33: [54, 62], 34: [0, 16], 35: [3, 9, 30, 31, 40]},
}
EMPTY_WINDOWS = (20, 21)
BACKGROUND_FIRST_WINDOW = 40
TARGET_NNZ = 200_000


def plan(nrows, ncols, cus):
    """(wbits, nwindows, ntiles, nsplit, tiles_per) of blocked_build / blocked_mxv_kernel."""
    wbits = 10
    while wbits < MAX_WBITS and (nrows >> wbits) > 256:
        wbits += 1
    nwindows = (nrows + (1 << wbits) - 1) >> wbits
    ntiles = (ncols + TILE - 1) >> TILE_BITS
    nsplit = 1
    while nwindows * nsplit < 2 * cus and nsplit < ntiles:
        nsplit <<= 1
    nsplit = min(nsplit, ntiles)
    tiles_per = (ntiles + nsplit - 1) // nsplit
    return wbits, nwindows, ntiles, nsplit, tiles_per


def bucket_counts(csr, wbits):
    """Stored entries per bucket, as an (nwindows * ntiles, 32) array."""
    nwindows = (csr.nrows + (1 << wbits) - 1) >> wbits
    ntiles = (csr.ncols + TILE - 1) >> TILE_BITS
    rows, cols = csr.pairs()
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    key = ((rows >> wbits) * ntiles + (cols >> TILE_BITS)) * 32 + (rows & 31)
    return np.bincount(key, minlength=nwindows * ntiles * 32).reshape(nwindows * ntiles, 32)


def padded_blocks(cnt):
    """Per block: entries after every bucket is rounded up to 4, and after the block is rounded up to 256."""
    quads = ((cnt + 3) & ~3).sum(axis=1)
    return quads, (quads + CHUNK - 1) & ~(CHUNK - 1)


def padded_entries(csr, wbits):
    """(total, nonempty_blocks, nblocks): what bk_pad_count_kernel + the scan make of the matrix."""
    cnt = bucket_counts(csr, wbits)
    quads, padded = padded_blocks(cnt)
    return int(padded.sum()), int((quads > 0).sum()), int(cnt.shape[0])


def unit_profile(nonempty, nsplit, tiles_per):
    """How the units (window, part) of blocked_mxv_kernel meet empty blocks.  nonempty: (nwindows, ntiles) bool.
    Returns a list of dicts, one per unit: w, part, c0, c1, kind in {"past", "dead", "idle", "live"} (range past ntiles /
    nothing in the range although the window has entries / nothing in the whole window / something to stream) and, for
    live units, lead / mid / trail = empty blocks before the first, between, and after the last non-empty block."""
    nwindows, ntiles = nonempty.shape
    out = []
    for w in range(nwindows):
        for part in range(nsplit):
            c0 = part * tiles_per
            c1 = min(c0 + tiles_per, ntiles)
            u = {"w": w, "part": part, "c0": c0, "c1": c1, "lead": 0, "mid": 0, "trail": 0, "blocks": 0}
            if c0 >= ntiles:
                u["kind"] = "past"
            else:
                idx = np.nonzero(nonempty[w, c0:c1])[0]
                if len(idx) == 0:
                    u["kind"] = "dead" if nonempty[w].any() else "idle"
                else:
                    u["kind"] = "live"
                    u["blocks"] = len(idx)
                    u["lead"] = int(idx[0])
                    u["trail"] = int(c1 - c0 - 1 - idx[-1])
                    u["mid"] = int(idx[-1] - idx[0] + 1 - len(idx))
            out.append(u)
    return out


def bits(n, ids):
    """oracle.bits_from_ids for millions of ids: the same words through packbits."""
    b = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    b[np.asarray(ids, dtype=np.int64)] = True
    return np.packbits(b, bitorder="little").view(U64)


class Case:
    """One graph: M (oracle.CSR, the streamed matrix), a = M' (what oracle.vxm multiplies) and the special places."""

    def __init__(self, name, n, M, special):
        self.name, self.n, self.M, self.special = name, n, M, special
        self.a = oracle.transpose(M)

    def rows_storing(self, col):
        return self.a.row(col)

    def frontiers(self):
        """The multi-bit frontiers of the issue, as (name, bits): the last tile's columns, the columns of a tile that is
        empty in one hole window, a random fifth of the vertices, everything."""
        n, ntiles = self.n, (self.n + TILE - 1) >> TILE_BITS
        rng = np.random.default_rng(len(self.name) * 1000 + 5)
        c = self.special["empty_tile_probe"][1]
        return [
            ("last_tile", bits(n, np.arange((ntiles - 1) * TILE, n))),
            ("empty_tile", bits(n, np.arange(c * TILE, min((c + 1) * TILE, n)))),
            ("fifth", bits(n, rng.choice(n, n // 5, replace=False))),
            ("full", bits(n, np.arange(n))),
        ]

    def mask(self):
        rng = np.random.default_rng(len(self.name) * 1000 + 3)
        return bits(self.n, rng.choice(self.n, self.n // 3, replace=False))


class _Builder:
    def __init__(self, n, seed):
        self.n, self.rows, self.cols = n, [], []
        self.rng = np.random.default_rng(seed)

    def add(self, rows, cols):
        rows, cols = np.broadcast_arrays(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))
        assert rows.min() >= 0 and rows.max() < self.n and cols.min() >= 0 and cols.max() < self.n
        self.rows.append(rows.ravel().copy())
        self.cols.append(cols.ravel().copy())

    def tile_range(self, c):
        return c * TILE, min((c + 1) * TILE, self.n)

    def pick(self, c, k):
        """k distinct columns of tile c, sorted."""
        lo, hi = self.tile_range(c)
        return np.sort(lo + self.rng.choice(hi - lo, k, replace=False))

    def csr(self):
        return oracle.build_csr(self.n, self.n, np.concatenate(self.rows).astype(U64), np.concatenate(self.cols).astype(U64))


def background_tiles(w, ntiles):
    """The tiles of window w that receive background entries: a fixed pattern with holes."""
    return [c for c in range(ntiles) if (w * 7 + c * 3) % 5 != 0]


@functools.lru_cache(maxsize=None)
def make_case(name):
    n = CASES[name]
    wbits, nwindows, ntiles, _, _ = plan(n, n, 256)     # (wbits, nwindows and ntiles do not depend on the CU count)
    W = 1 << wbits
    b = _Builder(n, {"ragged4": 4, "split5": 5, "wide17": 17}[name])
    sp = {"cols": {}, "empty_windows": list(EMPTY_WINDOWS), "hole_windows": HOLE_WINDOWS[name]}
    cols = sp["cols"]                                    # name -> column of a one-bit frontier
    mid = min(1, ntiles - 1)

    # corners: the first row meets the last column, the last row the first and the last column.  Window 0 holds nothing
    # else, so block (0, ntiles - 1) is a one-entry block in a row with row & 31 == 0 as well.
    b.add([0, n - 1, n - 1], [n - 1, 0, n - 1])
    cols["last_col"], cols["first_col"] = n - 1, 0
    # the two sides of the first tile boundary, in one row
    sp["tile_edge_row"] = 2 * W + 9
    b.add([2 * W + 9, 2 * W + 9], [TILE - 1, TILE])
    cols["tile0_last"], cols["tile1_first"] = TILE - 1, TILE
    # the last row of a window (output word (W >> 5) - 1, bit 31: word 4095 at wbits 17) and the first row of the next
    e = b.pick(mid, 2)
    sp["window_edge_rows"] = (5 * W + W - 1, 6 * W)
    b.add([5 * W + W - 1, 6 * W], e)
    cols["window_last_row"], cols["window_first_row"] = int(e[0]), int(e[1])

    # hubs: 5 000 entries over all tiles (1 000 of them in tile 0), and 3 000 in tile 0 in row hub + 32: same window, same
    # row & 31, so the 64-entry chunks of the two rows land in one bucket in whatever order the atomics decide
    hub = 10 * W + 7
    base = np.unique(np.concatenate([b.pick(0, 1000)] + [b.pick(c, 8) for c in range(1, ntiles)]))
    extra = b.rng.choice(n, 8000, replace=False)
    extra = extra[~np.isin(extra, base)][: 5000 - len(base)]
    hub_cols = np.sort(np.concatenate([base, extra]))
    hub2_cols = b.pick(0, 3000)
    b.add(hub, hub_cols)
    b.add(hub + 32, hub2_cols)
    sp["hubs"] = (hub, hub + 32)
    in0 = hub_cols[hub_cols < TILE]
    cols["hub_tile0_mid"] = int(in0[len(in0) // 2 + 1])          # inside a run of lanes, not at its head
    cols["hub_last_tile"] = int(hub_cols[-1])
    cols["hub2_mid"] = int(hub2_cols[1501])

    # short rows: r and r + 32 (one bucket) with k entries each in one tile -> quads that mix two output words
    short = []
    for i, (k0, k1) in enumerate([(1, 1), (2, 2), (3, 3), (5, 5), (1, 5)]):
        r = 12 * W + 64 * i + 3 + i
        c0, c1 = b.pick(mid, k0), b.pick(mid, k1)
        b.add(r, c0)
        b.add(r + 32, c1)
        short.append((r, r + 32, k0, k1, mid))
        cols[f"short{k0}{k1}_r"], cols[f"short{k0}{k1}_r32"] = int(c0[0]), int(c1[-1])
    sp["short_rows"] = short

    # a block whose only entry sits in a row with row & 31 == 0: bucket 0 takes 3 pads, the empty bucket 31 the other 252
    one_c = min(2, ntiles - 1)
    one = b.pick(one_c, 1)
    b.add(14 * W + 64, one)
    sp["one_entry_block"] = (14, one_c, 14 * W + 64)
    cols["one_entry"] = int(one[0])
    # exact sizes, from whole rows of 4 k entries in one bucket: 256 entries (no pad at all), and 256 + 1
    b.add(16 * W + 5, b.pick(mid, 256))
    b.add(17 * W + 5, b.pick(mid, 256))
    lone = b.pick(mid, 1)
    b.add(17 * W + 38, lone)
    sp["exact256"], sp["exact257"] = (16, mid), (17, mid)
    cols["exact257_lone"] = int(lone[0])
    # 253 + 1 entries in two buckets: 256 + 4 after the buckets are rounded to quads, so the block takes 512 entries where
    # 254 unrounded ones would take 256: the reported entry count tells whether the builder rounds buckets
    b.add(18 * W + 5, b.pick(mid, 253))
    b.add(18 * W + 38, b.pick(mid, 1))
    sp["quad_rounding_block"] = (18, mid)

    # hole windows: 40 entries in each listed tile and nothing else
    for w, tiles in HOLE_WINDOWS[name].items():
        for c in tiles:
            cc = b.pick(c, 40)
            b.add(w * W + b.rng.integers(0, W, len(cc)), cc)
        cols[f"hole{w}"] = int(cc[0])
    w0 = min(HOLE_WINDOWS[name])
    sp["empty_tile_probe"] = (w0, next(c for c in range(ntiles) if c not in HOLE_WINDOWS[name][w0]))

    # background: the rest of the ~200 000 entries, confined to background_tiles() of the windows from 40 on
    blocks = [(w, c) for w in range(BACKGROUND_FIRST_WINDOW, nwindows) for c in background_tiles(w, ntiles)]
    per = (TARGET_NNZ - sum(len(r) for r in b.rows)) // len(blocks)
    for w, c in blocks:
        lo, hi = b.tile_range(c)
        b.add(b.rng.integers(w * W, min((w + 1) * W, n), per), b.rng.integers(lo, hi, per))
    sp["background_blocks"] = blocks
    return Case(name, n, b.csr(), sp)


def check_preconditions(case, cus):
    """Assert that `case` reaches, under the plan for `cus` compute units, every path it was built for.  Returns the
    figures it looked at (the CPU test prints them)."""
    name, n, M, sp = case.name, case.n, case.M, case.special
    wbits, nwindows, ntiles, nsplit, tiles_per = pl = plan(n, n, cus)
    if (name, cus) in EXPECTED_PLAN:
        assert pl == EXPECTED_PLAN[(name, cus)], pl
    W = 1 << wbits
    deg = np.diff(M.rowptr.astype(np.int64))
    cnt = bucket_counts(M, wbits)
    quads, padded = padded_blocks(cnt)
    raw = cnt.sum(axis=1)
    nonempty = (raw > 0).reshape(nwindows, ntiles)
    blk = lambda w, c: w * ntiles + c
    fig = {"plan": pl, "nnz": M.nnz, "units": nwindows * nsplit}

    assert 180_000 <= M.nnz <= 220_000, M.nnz
    # ragged: the last tile and the last window are cut, and y ends inside the last window
    assert n % TILE != 0 and n % W != 0 and (n + 63) // 64 < nwindows * (W // 64)
    if name == "ragged4":
        assert n - (ntiles - 1) * TILE == 777
    # more units than any grid the launch picks (at most two workgroups per CU): some workgroup walks a second unit
    assert nwindows * nsplit > 2 * cus, (nwindows * nsplit, cus)
    assert nsplit > 1                                    # several workgroups flush into one window
    for w in sp["empty_windows"]:
        assert not nonempty[w].any()
    assert len(sp["empty_windows"]) >= 2
    for w, tiles in sp["hole_windows"].items():
        assert np.nonzero(nonempty[w])[0].tolist() == sorted(tiles), (w, tiles)

    # how the units meet empty blocks
    units = unit_profile(nonempty, nsplit, tiles_per)
    live = [u for u in units if u["kind"] == "live"]
    kinds = {k: sum(u["kind"] == k for u in units) for k in ("live", "dead", "idle", "past")}
    fig.update(kinds=kinds, lead=sum(u["lead"] > 0 for u in live), mid=sum(u["mid"] > 0 for u in live),
               trail=sum(u["trail"] > 0 for u in live), multi=sum(u["blocks"] > 1 for u in live))
    assert kinds["dead"] >= 1 and kinds["idle"] >= 2               # `any == false`, in a live and in an empty window
    if name == "ragged4":
        assert tiles_per == 1
    else:
        assert tiles_per > 1
        assert fig["multi"] >= 1                          # the pipeline crosses a tile inside a unit
        hole = [u for u in live if u["w"] in sp["hole_windows"]]
        span = lambda u: u["c1"] - u["c0"]
        assert any(u["blocks"] == 1 and u["lead"] == span(u) - 1 and span(u) > 1 for u in hole), "only the last tile"
        assert any(u["blocks"] == 1 and u["trail"] == span(u) - 1 and span(u) > 1 for u in hole), "only the first tile"
    if name == "split5":
        assert kinds["past"] == nwindows                  # one part's range lies past ntiles
        assert any(u["c1"] - u["c0"] == 1 for u in units if u["kind"] != "past")   # and one part has one tile
    if name == "wide17":
        assert wbits == MAX_WBITS
        hole = [u for u in live if u["w"] in sp["hole_windows"]]
        assert any(u["blocks"] == 2 and u["lead"] == 0 and u["trail"] == 0 and u["mid"] >= 1 for u in hole), "first and last only"
        assert fig["lead"] >= 1 and fig["mid"] >= 1 and fig["trail"] >= 1

    # hubs
    hub, hub2 = sp["hubs"]
    assert deg[hub] == 5000 and deg[hub2] == 3000 and hub2 == hub + 32 and (hub >> wbits) == (hub2 >> wbits)
    assert len(np.unique(M.row(hub) >> U64(TILE_BITS))) == ntiles
    assert int(M.row(hub2).max()) < TILE
    hub_in0 = int((M.row(hub) < TILE).sum())
    assert hub_in0 > 64 and cnt[blk(hub >> wbits, 0), hub & 31] == hub_in0 + 3000     # chunks of both rows in one bucket
    fig["hub_bucket"] = hub_in0 + 3000
    # short rows: both rows of a pair in one bucket and nothing else there
    for r, r32, k0, k1, c in sp["short_rows"]:
        assert deg[r] == k0 and deg[r32] == k1 and (r & 31) == (r32 & 31) and (r >> 5) != (r32 >> 5)
        assert cnt[blk(r >> wbits, c), r & 31] == k0 + k1
    assert sorted({(k0, k1) for _, _, k0, k1, _ in sp["short_rows"]}) == [(1, 1), (1, 5), (2, 2), (3, 3), (5, 5)]
    # one-entry block in a row with row & 31 == 0: the pads of bucket 31 come from an empty bucket
    w, c, r = sp["one_entry_block"]
    assert raw[blk(w, c)] == 1 and cnt[blk(w, c), 0] == 1 and (r & 31) == 0 and padded[blk(w, c)] == CHUNK
    assert raw[blk(0, ntiles - 1)] == 1                   # (the corner (0, n - 1) is another)
    # exact sizes
    w, c = sp["exact256"]
    assert raw[blk(w, c)] == 256 and quads[blk(w, c)] == 256 and padded[blk(w, c)] == 256
    w, c = sp["exact257"]
    assert raw[blk(w, c)] == 257 and quads[blk(w, c)] == 260 and padded[blk(w, c)] == 512
    w, c = sp["quad_rounding_block"]
    assert raw[blk(w, c)] == 254 and quads[blk(w, c)] == 260 and padded[blk(w, c)] == 512
    # corners and edges
    for r, c in [(0, n - 1), (n - 1, 0), (n - 1, n - 1), (sp["tile_edge_row"], TILE - 1), (sp["tile_edge_row"], TILE)]:
        assert M.has_edges([r], [c])[0], (r, c)
    r_last, r_first = sp["window_edge_rows"]
    assert deg[r_last] >= 1 and deg[r_first] >= 1 and r_last + 1 == r_first and (r_last >> wbits) + 1 == (r_first >> wbits)
    assert (r_last & 31) == 31 and ((r_last & (W - 1)) >> 5) == (W >> 5) - 1          # output word 4095 at wbits 17
    # the probe tile of the "empty-in-that-window" frontier is empty there and used elsewhere
    w, c = sp["empty_tile_probe"]
    assert nonempty[w].any() and not nonempty[w, c] and nonempty[:, c].any()
    # blocks whose empty last bucket is padded (the n == 0 branch of bk_pad_fill_kernel)
    fig["pad_from_empty_last_bucket"] = int(((raw > 0) & (cnt[:, 31] == 0) & (padded > quads)).sum())
    assert fig["pad_from_empty_last_bucket"] >= 2
    # every one-bit frontier names a stored column
    for k, col in sp["cols"].items():
        assert len(case.rows_storing(col)) >= 1, k
    fig["one_bit_frontiers"] = len(sp["cols"])
    return fig
