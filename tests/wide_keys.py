"""Case builders and plain numpy references for the stable sorts and builders of the matrix layer on wide id spaces
(tests/test_gpu_wide_keys.py runs them on the device, tests/test_wide_keys_cpu.py holds the builders to what they claim).

The sorts of transpose.hip shape themselves by the WIDTH of the key space (falkordb_amd/csrc/sort_plan.hpp), their memory by
the width too and not by the entry count: a few thousand entries reach every shape.  Everything here is deterministic, pure
numpy at 64 bits — np.lexsort on (row, col), dicts filled in input order — and shares nothing with the device code or with the
C oracle."""
import numpy as np

U64 = np.uint64
LADDER = (1 << 22, (1 << 24) + 1, 1 << 26, (1 << 26) + 1, 1 << 27, (1 << 27) + 1)
NARROW = 300                   # the other dimension of a ladder matrix
HEAVY = 300                    # entries that carry one key
NKEYS_ENTRIES = 5000           # entries of a key set
TWO_LEVEL_MAX = 1 << 26        # the widest key space the two-level form takes (8192 buckets of 2^13 keys)


def u64(x):
    return np.ascontiguousarray(x, dtype=U64)


def key_bits(nkeys):
    """The smallest kb >= 1 with 2^kb >= nkeys."""
    return max(1, int(nkeys - 1).bit_length())


def staged_levels(nkeys):
    """Levels of the LDS-staged form: 9 bits a level, three from 17 bits."""
    kb = key_bits(nkeys)
    return max((kb + 8) // 9, 3 if kb >= 17 else 1)


def heavy_key(nkeys):
    return nkeys // 3 + 1


_groups = {}


def key_groups(nkeys):
    """The groups of a width's key set, by name: both ends of the key space, both sides of every digit boundary whatever the
    split (2^j - 1, 2^j and nkeys - 1 - 2^j for every bit j), one key carried by HEAVY entries, seeded random keys."""
    if nkeys not in _groups:
        kb = key_bits(nkeys)
        g = {"low": np.arange(64), "high": np.arange(nkeys - 64, nkeys),
             "bits": np.array([k for j in range(kb) for k in ((1 << j) - 1, 1 << j, nkeys - 1 - (1 << j))]),
             "heavy": np.full(HEAVY, heavy_key(nkeys))}
        rest = NKEYS_ENTRIES - sum(len(x) for x in g.values())
        rnd = np.random.default_rng(nkeys).integers(0, nkeys, rest)
        rnd[rnd == heavy_key(nkeys)] = 0
        g["random"] = rnd
        _groups[nkeys] = {k: u64(v) for k, v in g.items()}
    return _groups[nkeys]


def key_set(nkeys):
    """NKEYS_ENTRIES keys below nkeys, the groups one after the other; entry i of the heavy group is entry heavy_slice.start + i."""
    return np.concatenate(list(key_groups(nkeys).values()))


def heavy_slice(nkeys):
    g = key_groups(nkeys)
    a = sum(len(g[k]) for k in ("low", "high", "bits"))
    return slice(a, a + HEAVY)


def narrow_ids(nkeys):
    """The narrow coordinate of every entry of the key set: 0 .. HEAVY - 1 in order on the heavy key — only a stable sort leaves
    them ascending —, a scramble of the position elsewhere."""
    i = np.arange(NKEYS_ENTRIES)
    out = (i * 7919 + 13) % NARROW
    hs = heavy_slice(nkeys)
    out[hs] = np.arange(HEAVY)
    return u64(out)


def value_of(r, c, salt=0):
    """A value distinct per coordinate, top bit in use."""
    return (u64(r) * U64(1_000_003) + u64(c) * U64(7) + U64(salt)) | (U64(1) << U64(63))


def sort_unique(rows, cols):
    """(rows, cols) in storage order — by row, then column, at 64 bits — with duplicates collapsed."""
    rows, cols = u64(rows), u64(cols)
    o = np.lexsort((cols, rows))
    r, c = rows[o], cols[o]
    keep = np.ones(len(r), dtype=bool)
    keep[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    return r[keep], c[keep]


def last_wins(rows, cols, vals):
    """{(row, col): value of the LAST tuple of that coordinate in input order} — a dict filled in order."""
    d = {}
    for r, c, v in zip(u64(rows).tolist(), u64(cols).tolist(), u64(vals).tolist()):
        d[(r, c)] = v
    return d


def csr_of(nrows, rows, cols):
    """(rowptr, colidx) of sorted-unique coordinates; only for a small nrows."""
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows.astype(np.int64), minlength=nrows))])
    return u64(rp), u64(cols)


_cases = {}


def _cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _cases:
            _cases[k] = fn(*key)
        return _cases[k]
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


@_cached
def transpose_case(nkeys):
    """The NARROW x nkeys pattern whose columns are the key set: dict(rowptr, colidx, vals, rows, cols) — rows / cols the
    coordinates in storage order, vals their values — and t_rows / t_cols / t_vals of its transpose."""
    r, c = sort_unique(narrow_ids(nkeys), key_set(nkeys))
    rp, ci = csr_of(NARROW, r, c)
    tr, tc = sort_unique(c, r)
    return dict(rowptr=rp, colidx=ci, rows=r, cols=c, vals=value_of(r, c), t_rows=tr, t_cols=tc, t_vals=value_of(tc, tr))


COO_SHAPES = ("tall", "wide", "square")


@_cached
def coo_case(nkeys, shape):
    """NKEYS_ENTRIES + 700 shuffled tuples, 700 of them repeats of earlier coordinates (the heavy key's among them), each with a
    value of its own: dict(nrows, ncols, rows, cols, vals) and the reference — ref_rows / ref_cols in storage order, ref_vals
    where the LAST tuple of a coordinate wins.  tall: nkeys x NARROW; wide: NARROW x nkeys; square: nkeys x nkeys, the columns
    being the key set in another order."""
    rng = np.random.default_rng(nkeys + COO_SHAPES.index(shape))
    keys, small = key_set(nkeys), narrow_ids(nkeys)
    if shape == "tall":
        nrows, ncols, r, c = nkeys, NARROW, keys, small
    elif shape == "wide":
        nrows, ncols, r, c = NARROW, nkeys, small, keys
    else:
        nrows, ncols, r, c = nkeys, nkeys, keys, np.roll(keys[::-1], 1234)
    again = np.concatenate([np.arange(heavy_slice(nkeys).start, heavy_slice(nkeys).start + 200), rng.integers(0, NKEYS_ENTRIES, 500)])
    r, c = np.concatenate([r, r[again]]), np.concatenate([c, c[again]])
    p = rng.permutation(len(r))
    r, c = u64(r[p]), u64(c[p])
    v = u64(np.arange(len(r))) * U64(0x9E3779B97F4A7C15) + U64(1)
    rr, rc = sort_unique(r, c)
    want = last_wins(r, c, v)
    rv = u64([want[k] for k in zip(rr.tolist(), rc.tolist())])
    return dict(nrows=nrows, ncols=ncols, rows=r, cols=c, vals=v, ref_rows=rr, ref_cols=rc, ref_vals=rv)


EDGE_SIDES = ("rows", "cols")
MULTI = 2 ** 64 - 1


@_cached
def edges_case(nkeys, side):
    """A bulk batch whose sources (side "rows") or destinations ("cols") are the key set, with 700 further tuples on pairs that
    exist already: dict(nrows, ncols, srcs, dsts, ids) and the reference of a plain dict pair -> ascending ids: fwd_rows /
    fwd_cols / fwd_vals (the id, or MULTI for a pair with several), bwd_rows / bwd_cols, multi_key, multi_off, multi_ids."""
    c = coo_case(nkeys, "tall" if side == "rows" else "wide")
    s, d = c["rows"], c["cols"]
    ids = u64(np.random.default_rng(nkeys + 77).permutation(len(s))) + U64(1 << 40)
    pairs = {}
    for a, b, i in zip(s.tolist(), d.tolist(), ids.tolist()):
        pairs.setdefault((a, b), []).append(i)
    order = sorted(pairs)
    for v in pairs.values():
        v.sort()
    multi = [p for p in order if len(pairs[p]) > 1]
    br, bc = sort_unique([p[1] for p in order], [p[0] for p in order])
    return dict(nrows=c["nrows"], ncols=c["ncols"], srcs=s, dsts=d, ids=ids,
                fwd_rows=u64([p[0] for p in order]), fwd_cols=u64([p[1] for p in order]),
                fwd_vals=u64([pairs[p][0] if len(pairs[p]) == 1 else MULTI for p in order]), bwd_rows=br, bwd_cols=bc,
                multi_key=u64([(a << 32) | b for a, b in multi]),
                multi_off=u64(np.concatenate([[0], np.cumsum([len(pairs[p]) for p in multi])])),
                multi_ids=u64([i for p in multi for i in pairs[p]]))


def probe_coords(rows, cols):
    """Every stored coordinate and its neighbours (r, c - 1), (r, c + 1), as 64-bit arrays (column 0 wraps to 2^64 - 1), and
    whether each is stored."""
    rows, cols = u64(rows), u64(cols)
    pr = np.concatenate([rows, rows, rows])
    pc = np.concatenate([cols, cols - U64(1), cols + U64(1)])
    stored = set(zip(rows.tolist(), cols.tolist()))
    return pr, pc, np.array([k in stored for k in zip(pr.tolist(), pc.tolist())], dtype=np.uint8)


# ---- ids past 2^31 --------------------------------------------------------------------------------------------------------
HALF = 1 << 31
WIDE_ROWS = 70
TALL_NROWS = 2 ** 32 - 2


def marks(N):
    """The six positions of an id space past 2^31: both ends and both sides of bit 31."""
    return [0, HALF - 1, HALF, HALF + 1, N - 2, N - 1]


def run_across(N, before=65, after=64):
    return [k for k in range(HALF - before, HALF + after + 1) if k < N]


@_cached
def straddle_rows(N, salt):
    """{row: columns} of a WIDE_ROWS x N content: rows holding the six marks, a run across 2^31, both, and parts of either;
    rows 0, 63, 64, 65 and the last are populated.  Contents of different salts share rows and about half of their entries."""
    m, run = marks(N), run_across(N)
    rows = {0: m, 1: run, 5: m + run, 63: m[1:4], 64: run[::2] + [N - 1], 65: [HALF], 66: [HALF - 1], 67: [0, N - 1],
            WIDE_ROWS - 1: m + run[::3]}
    if salt:
        rng = np.random.default_rng(salt)
        rows = {r: sorted(set(c[::2]) | set(rng.choice(run + m, 9).tolist())) for r, c in rows.items() if r != 65}
        rows[2 + salt] = [HALF - 1, HALF, N - 1]
    return {r: sorted(set(c)) for r, c in rows.items()}


def coords_of(rows):
    """(rows, cols) of {row: columns} in storage order."""
    r = [x for x in sorted(rows) for _ in rows[x]]
    c = [y for x in sorted(rows) for y in sorted(rows[x])]
    return u64(r), u64(c)


def dense_arrays(nrows, rows):
    r, c = coords_of(rows)
    return csr_of(nrows, r, c)


def hyper_arrays(rows):
    """{row: columns} -> (short rowptr, colidx, hyper_rows) for mat_from_csr."""
    hr = sorted(rows)
    rp = np.concatenate([[0], np.cumsum([len(rows[r]) for r in hr])])
    return u64(rp), coords_of(rows)[1], u64(hr)


def as_set(rows):
    return {(r, c) for r, cs in rows.items() for c in cs}


def merged(m, dp, dm, dm_masks_dp=False):
    """(m minus dm) united with dp as a set of coordinates; dm also removes dp's entries when dm_masks_dp."""
    return (m - dm) | ((dp - dm) if dm_masks_dp else dp)


@_cached
def tall_rows(salt=0):
    """{row: columns} with TALL_NROWS = 2^32 - 2 rows over 1000 columns, stored rows at the six marks."""
    return {r: sorted({0, 5 + i + salt, 999 - salt}) for i, r in enumerate(marks(TALL_NROWS))}
