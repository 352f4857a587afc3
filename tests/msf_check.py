"""CPU checker of the minimum spanning forest for the MSF tests: Kruskal over the edge order include/fgpu.h writes down for
fgpu_msf.  Every unordered pair {v, w} is one edge with the key (K(bits), min, max); K is the IEEE totalOrder of the stored
binary64 bit pattern with -0.0 = +0.0.  The order is strict and total, so the forest is unique: the GPU tests compare by array
equality.  tests/test_msf_cpu.py holds this against an independent Boruvka."""
import numpy as np

U64 = np.uint64
SIGN = U64(0x8000000000000000)
ONE_BITS = U64(0x3FF0000000000000)


def key_of(bits):
    """K: -0.0 becomes +0.0, then every bit of a negative pattern flips and only the sign bit of a non-negative one."""
    b = np.array(bits, dtype=U64, copy=True).reshape(-1)
    b[b == SIGN] = U64(0)
    neg = (b >> U64(63)) != 0
    return np.where(neg, ~b, b ^ SIGN)


def bits_of(weights):
    return np.ascontiguousarray(weights, dtype=np.float64).view(U64)


def upper_pairs(rows, cols, bits=None, active=None):
    """The entries that count, once per pair as (lo < hi): the upper triangle of the symmetric matrix without the diagonal and
    without entries that have an inactive end.  bits None = a BOOL matrix, every weight 1.0."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    bits = np.full(len(rows), ONE_BITS, dtype=U64) if bits is None else np.asarray(bits, dtype=U64)
    keep = rows < cols
    if active is not None:
        active = np.asarray(active, dtype=bool)
        keep &= active[rows] & active[cols]
    return rows[keep], cols[keep], bits[keep]


def msf(n, rows, cols, bits=None, active=None):
    """(forest rows, forest cols, weight bits, component) of the symmetric matrix given by its stored entries (both directions
    of every pair): the forest as row < col sorted by (row, col), component[v] = the smallest id of v's tree, -1 if inactive."""
    lo, hi, b = upper_pairs(rows, cols, bits, active)
    order = np.lexsort((hi, lo, key_of(b)))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    took = []
    for i in order:
        a, c = find(int(lo[i])), find(int(hi[i]))
        if a != c:
            parent[max(a, c)] = min(a, c)
            took.append(i)
    took = np.array(took, dtype=np.int64)
    fr, fc, fb = lo[took], hi[took], b[took]
    o = np.lexsort((fc, fr))
    comp = np.array([find(v) for v in range(n)], dtype=np.int64)
    if active is not None:
        comp[~np.asarray(active, dtype=bool)] = -1
    return fr[o].astype(U64), fc[o].astype(U64), fb[o], comp


def components(comp):
    comp = np.asarray(comp)
    return int((comp == np.arange(len(comp))).sum())
