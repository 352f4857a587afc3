"""Case builders and plain numpy references for the matrix layer's size-class, threshold and form edges
(tests/test_gpu_matrix_edges.py runs them on the device, tests/test_matrix_edges_cpu.py checks the builders themselves).

Everything here is deterministic.  The references are plain numpy at full width — np.unique per row, set operations on the
linear key row * ncols + col, dicts for values — and share nothing with the device code or with the C oracle, which the CPU
test holds them against."""
import numpy as np

U64 = np.uint64


def u64(x):
    return np.ascontiguousarray(x, dtype=U64)


class Csr:
    """A sorted-unique CSR pattern on the host."""

    def __init__(self, nrows, ncols, rowptr, colidx):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.rowptr, self.colidx = u64(rowptr), u64(colidx)

    @property
    def nnz(self):
        return int(self.rowptr[-1])

    def row(self, r):
        return self.colidx[int(self.rowptr[r]):int(self.rowptr[r + 1])]

    def lengths(self):
        return np.diff(self.rowptr.astype(np.int64))

    def pairs(self):
        return np.repeat(np.arange(self.nrows, dtype=U64), self.lengths()), self.colidx.copy()

    def keys(self):
        r, c = self.pairs()
        return r * U64(self.ncols) + c

    def to_set(self):
        r, c = self.pairs()
        return set(zip(r.tolist(), c.tolist()))

    def hyper(self):
        """(short rowptr, hyper_rows): the hypersparse form mat_from_csr takes — the populated rows only."""
        deg = self.lengths()
        rows = np.nonzero(deg)[0]
        return u64(np.concatenate([[0], np.cumsum(deg[rows])])), u64(rows)


def from_keys(nrows, ncols, keys):
    """Csr of the coordinates whose linear keys (row * ncols + col) are given, in any order, duplicates allowed."""
    keys = np.unique(u64(keys))
    rows = (keys // U64(max(ncols, 1))).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))])
    return Csr(nrows, ncols, rowptr, keys % U64(max(ncols, 1)))


def build(nrows, ncols, rows, cols):
    return from_keys(nrows, ncols, u64(rows) * U64(ncols) + u64(cols))


def from_rows(nrows, ncols, rows):
    """Csr from {row: iterable of column ids}; every row goes through np.unique."""
    rp = np.zeros(nrows + 1, dtype=np.int64)
    chunks = []
    for r in sorted(rows):
        x = np.unique(u64(rows[r]))
        rp[r + 1] = len(x)
        chunks.append(x)
    return Csr(nrows, ncols, np.cumsum(rp), np.concatenate(chunks) if chunks else np.zeros(0, dtype=U64))


def transpose(a):
    r, c = a.pairs()
    return build(a.ncols, a.nrows, c, r)


def mxm(f, b):
    """Row i of F x B = the sorted union of the B-rows that F-row i names."""
    rows = {}
    for i in np.nonzero(f.lengths())[0].tolist():
        seg = np.concatenate([b.row(s) for s in f.row(i).tolist()])
        if len(seg):
            rows[i] = seg
    return from_rows(f.nrows, b.ncols, rows)


def merge(m, dp, dm, dm_masks_dp=False):
    """(m minus dm) united with dp; dm also removes dp's entries when dm_masks_dp."""
    km = m.keys()
    kp = dp.keys() if dp is not None else np.zeros(0, dtype=U64)
    kd = dm.keys() if dm is not None else np.zeros(0, dtype=U64)
    keep = np.setdiff1d(km, kd)
    add = np.setdiff1d(kp, kd) if dm_masks_dp else kp
    return from_keys(m.nrows, m.ncols, np.union1d(keep, add))


def intersect(a, b):
    return from_keys(a.nrows, a.ncols, np.intersect1d(a.keys(), b.keys()))


def clip(a, nrows, ncols, row_lo=0, col_lo=0):
    """The entries of `a` with row_lo <= row < nrows and col_lo <= col < ncols, in a's own dimensions."""
    r, c = a.pairs()
    k = (r >= row_lo) & (r < nrows) & (c >= col_lo) & (c < ncols)
    return build(a.nrows, a.ncols, r[k], c[k])


def resize(a, nrows, ncols):
    r, c = a.pairs()
    k = (r < nrows) & (c < ncols)
    return build(nrows, ncols, r[k], c[k])


def last_wins(rows, cols, vals):
    """{(row, col): value of the LAST tuple of that coordinate in input order} — a dict filled in order."""
    d = {}
    for r, c, v in zip(u64(rows).tolist(), u64(cols).tolist(), u64(vals).tolist()):
        d[(r, c)] = v
    return d


def value_of(r, c, salt=0):
    """The value every valued case stores at (r, c): distinct per coordinate, top bit in use."""
    return (u64(r) * U64(1_000_003) + u64(c) * U64(7) + U64(salt)) | (U64(1) << U64(63))


# ---- 1. sort-and-unique classes ----------------------------------------------------------------------------------------
SORT_LENGTHS = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
SORT_PATTERNS = ("interleave", "below", "identical", "ends")
KEY_SPACES = (4100, 10007, (1 << 20) + 3)
WIDE_KEY_SPACES = ((1 << 31) + 5, (1 << 32) - 2)   # column ids with bit 31 set, up to the largest legal one (numpy reference only)
DUP_COUNTS = (64, 65, 4097)


def sort_pair(L, pattern, N):
    """Two sorted-unique key rows whose lengths add up to L, and the unique count their union must have.
    interleave: evens / odds spread over the key space; below: every key of the second row below the first row's;
    identical: the same row twice (an odd L gives the second row one key more); ends: a run from key 0 and a run up to
    key N - 1.  Where L exceeds the key space the disjoint patterns overlap instead and the union is the whole space."""
    h1, h2 = (L + 1) // 2, L // 2
    ar = np.arange
    if pattern == "identical":
        s = max(1, (N - 2) // max(1, h2))
        x = ar(h2) * s + 1
        return u64(x), u64(np.concatenate([[0], x]) if L & 1 else x), h1
    if L > N:                                                   # (8193 keys over 4100 columns)
        lo, hi = ar(h1), ar(N - h2, N)
        return (u64(hi), u64(lo), N) if pattern == "below" else (u64(lo), u64(hi), N)
    s = max(1, (N - 1) // L)
    if pattern == "interleave":
        return u64(ar(h1) * 2 * s), u64((ar(h2) * 2 + 1) * s), L
    if pattern == "below":
        return u64(N - 1 - ar(h1)[::-1] * s), u64(ar(h2) * s), L
    if pattern == "ends":
        return u64(ar(h1)), u64(ar(N - h2, N)), L
    raise ValueError(pattern)


class SortCases:
    """All sort-class cases of one key space packed into ONE product F x B.

    B holds two rows per (L, pattern) case and DUP_COUNTS[-1] rows with the same single key; F has one row per case — two
    entries naming the pair, or 64 / 65 / 4097 entries naming single-key rows — shuffled, and separated by empty rows and
    by single-entry rows.  `claims[i]` = (name, L, unique) for the F-rows that are cases, `parts[i]` the B-rows F-row i
    gathers, in order.  C is the expected product."""

    def __init__(self, N):
        self.N = N
        brows, cases = [], []
        for L in SORT_LENGTHS:
            for pat in SORT_PATTERNS:
                a, b, uniq = sort_pair(L, pat, N)
                cases.append((f"L{L}-{pat}", L, uniq, [len(brows), len(brows) + 1]))
                brows += [a, b]
        dup0 = len(brows)
        self.dup_key = N // 3
        brows += [u64([self.dup_key])] * DUP_COUNTS[-1]
        for d in DUP_COUNTS:
            cases.append((f"dup{d}", d, 1, list(range(dup0, dup0 + d))))
        rng = np.random.default_rng(N)
        order = rng.permutation(len(cases)).tolist()
        frows, self.claims = [], {}
        for n, ci in enumerate(order):
            name, L, uniq, ids = cases[ci]
            self.claims[len(frows)] = (name, L, uniq)
            frows.append(ids)
            single = [int(rng.integers(0, len(brows)))]
            frows += ([[]], [single], [[], single])[n % 3]
        while len(frows) % 64 != 1:                               # nrows + 1 just past a multiple of 64
            frows.append([])
        self.B = from_rows(len(brows), N, dict(enumerate(brows)))
        self.F = from_rows(len(frows), len(brows), {i: x for i, x in enumerate(frows) if x})
        self.parts = [[brows[j] for j in x] for x in frows]
        self.C = from_rows(len(frows), N, {i: np.concatenate(p) for i, p in enumerate(self.parts) if p})

    def segment(self, i):
        """The keys the product gathers for F-row i, duplicates included, before the sort."""
        return np.concatenate(self.parts[i]) if self.parts[i] else np.zeros(0, dtype=U64)

    def coo(self):
        """The gathered segments as COO tuples in a shuffled order: a build whose row lengths are the L's."""
        rows = np.concatenate([np.full(len(self.segment(i)), i, dtype=U64) for i in range(self.F.nrows)])
        cols = np.concatenate([self.segment(i) for i in range(self.F.nrows)])
        p = np.random.default_rng(self.N + 1).permutation(len(rows))
        return rows[p], cols[p]

    def layers(self):
        """(m, dp, dm): row i of m is the first B-row of F-row i, of dp the union of the others, so that a dirty row has
        len_m + len_dp = L; dm takes every third key of every second row."""
        m, dp, dm = {}, {}, {}
        for i, p in enumerate(self.parts):
            if p:
                m[i] = p[0]
            if len(p) > 1:
                dp[i] = np.concatenate(p[1:])
            if p and i % 2 == 0:
                dm[i] = np.unique(np.concatenate(p))[::3]
        n = self.F.nrows
        return from_rows(n, self.N, m), from_rows(n, self.N, dp), from_rows(n, self.N, dm)


_sort_cases = {}


def sort_cases(N):
    if N not in _sort_cases:
        _sort_cases[N] = SortCases(N)
    return _sort_cases[N]


# ---- 2. scan boundaries --------------------------------------------------------------------------------------------------
SCAN_TILE = 4096
SCAN_NROWS = (4095, 4096, 4097, 8191, 8192, 8193)
SCAN_NCOLS = 300
HUGE_NROWS = (1 << 24) + 4097               # nrows + 1 > 4096^2: the three-level scan
HUGE_NCOLS = 1000


def scan_rows(nrows):
    """Row 0, two rows on each side of every tile edge of the nrows + 1 scanned counts, the last row, two sparse ones."""
    rows = {0, nrows - 1, nrows // 3, nrows // 2 + 1}
    for t in range(SCAN_TILE, nrows + 2, SCAN_TILE):
        rows |= {t - 2, t - 1, t, t + 1}
    return sorted(r for r in rows if 0 <= r < nrows)


def scan_case(nrows):
    """(a, p, d, b): a / p / d of nrows x SCAN_NCOLS populated on scan_rows only (p shares half of a's entries, d removes
    from both), and b of SCAN_NCOLS x 200 for the product a x b."""
    rng = np.random.default_rng(nrows)
    lens = (1, 3, 70, 64, 65)
    a, p, d = {}, {}, {}
    for n, r in enumerate(scan_rows(nrows)):
        x = np.sort(rng.choice(SCAN_NCOLS, lens[n % 5], replace=False))
        a[r] = x
        p[r] = np.concatenate([x[::2], rng.integers(0, SCAN_NCOLS, 5)])
        d[r] = np.concatenate([x[1::3], p[r][-2:]])
    br, bc = rng.integers(0, SCAN_NCOLS, 2000), rng.integers(0, 200, 2000)
    return (from_rows(nrows, SCAN_NCOLS, a), from_rows(nrows, SCAN_NCOLS, p), from_rows(nrows, SCAN_NCOLS, d),
            build(SCAN_NCOLS, 200, br, bc))


def huge_case():
    """Two hypersparse contents of HUGE_NROWS rows as {row: sorted columns}, about a dozen entries each."""
    n = HUGE_NROWS
    rows = (0, 4095, 4096, (1 << 24) - 1, 1 << 24, n - 1)
    a = {r: [0, 5 + i, 999] for i, r in enumerate(rows)}
    b = {r: [0, 5 + i, 998] for i, r in enumerate(rows[::2])}
    b[4095] = [999]
    b[12345] = [7]
    return a, b


def hyper_arrays(rows):
    """{row: columns} -> (short rowptr, colidx, hyper_rows) for mat_from_csr."""
    hr = sorted(rows)
    rp = np.concatenate([[0], np.cumsum([len(rows[r]) for r in hr])])
    return u64(rp), u64(np.concatenate([np.sort(u64(rows[r])) for r in hr])), u64(hr)


# ---- 3. thresholds ----------------------------------------------------------------------------------------------------------
THRESHOLD_N = (4095, 4096, 4097)
TRANSPOSE_NCOLS = (1, 2, (1 << 17) - 1, 1 << 17, (1 << 17) + 1)


def heavy_dup_coo(n):
    """n tuples over 50 x 50 (almost every one a duplicate) with a distinct value per tuple."""
    rng = np.random.default_rng(n)
    return (rng.integers(0, 50, n, dtype=U64), rng.integers(0, 50, n, dtype=U64),
            u64(np.arange(n)) * U64(0x9E3779B97F4A7C15) + U64(1))


def transpose_case(nnz, ncols):
    """(nrows, rows, cols): exactly nnz DISTINCT coordinates in a shuffled order, so that the tuple count and the entry
    count both sit on the threshold; row 0, the last row, column 0 and the last column are in use."""
    nrows = max(64, (nnz + ncols - 1) // ncols + (900 if ncols <= 2 else 0))
    rng = np.random.default_rng(nnz * 31 + ncols)
    corners = np.unique(u64([0, ncols - 1, (nrows - 1) * ncols, nrows * ncols - 1]))
    lin = rng.choice(nrows * ncols, nnz, replace=False).astype(U64)
    lin = np.unique(np.concatenate([corners, lin]))
    keep = np.concatenate([corners, rng.permutation(np.setdiff1d(lin, corners))])[:nnz]
    keep = rng.permutation(keep)
    return nrows, keep // U64(ncols), keep % U64(ncols)


def thin_case(nrows, ncols):
    """6000 tuples over a 1 x N or N x 1 matrix: 5000 distinct coordinates, among them both ends, and 1000 repeats."""
    n = max(nrows, ncols)
    rng = np.random.default_rng(n + nrows)
    ids = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), 4998, replace=False)]).astype(U64)
    ids = rng.permutation(np.concatenate([ids, ids[:1000]]))
    zero = np.zeros(len(ids), dtype=U64)
    return (zero, ids) if nrows == 1 else (ids, zero)


def hyper_flip_coo(n_rows_populated, with_last_row=None):
    """3 tuples in each of n populated rows within 0 .. 4095 (row 0 and row 4095 among them); with_last_row adds one
    more populated row."""
    rng = np.random.default_rng(n_rows_populated)
    rows = np.concatenate([[0, 4095], rng.choice(np.arange(1, 4095), n_rows_populated - 2, replace=False)])
    if with_last_row is not None:
        rows = np.concatenate([rows, [with_last_row]])
    rows = np.repeat(u64(rows), 3)
    cols = u64((rows * U64(37) + u64(np.arange(len(rows)) % 3) * U64(1000)) % U64(4096))
    return rows, cols


# ---- 4. one content, two forms --------------------------------------------------------------------------------------------
FORM_N = 5000
FORMS = ("dense", "hyper")
FORM_PAIRS = tuple((a, b) for a in FORMS for b in FORMS)


def form_content(salt):
    """A square FORM_N content with 36 populated rows — row 0, the rows around 4096, the last row — whose lengths run over
    1, 63, 64, 65, 129, 2, 7, 300.  Contents of different salts share rows and half of their entries."""
    rng = np.random.default_rng(1234)
    rows = np.unique(np.concatenate([[0, 1, 4095, 4096, FORM_N - 1], rng.choice(FORM_N, 31, replace=False)]))
    lens = (1, 63, 64, 65, 129, 2, 7, 300)
    out = {}
    for n, r in enumerate(rows.tolist()):
        base = np.sort(rng.choice(FORM_N, lens[n % 8], replace=False))
        if salt == 0 or n % 7 == 3:
            out[r] = base
        elif n % 7 != 5:                                           # (rows with n % 7 == 5 exist in salt 0 only)
            mine = np.random.default_rng(salt * 1000 + n).choice(FORM_N, lens[(n + salt) % 8], replace=False)
            out[r] = np.concatenate([base[::2], mine])
    if salt:
        out[2 + salt] = [0, FORM_N - 1]                            # a row salt 0 leaves empty
    return from_rows(FORM_N, FORM_N, out)
