"""numpy model of the count hop's hub set and of a whole-frontier call's tiered passes (bitpart.hip bp_xplan_hub_set_build,
spgemm.hip scan_strong_first): what tests/test_gpu_xp_hub_set.py expects of the device, checked on its own in
tests/test_xp_hub_set_model.py.

H = the rows whose out-degree is at least a quarter of the largest one (rounded up), by (degree descending, id ascending), the
first 32.  A second reduced plan exists when |H| >= 2, out(H[0]) holds at least a quarter of the entries of A' (the first reduced
plan's rule) and the rows of the union of out(H[i]) outside out(H[0]) hold at least an eighth."""
import numpy as np

I64 = np.int64
DEG_DEN, SET_MAX, HUB_SHARE_DEN, SET_SHARE_DEN = 4, 32, 4, 8
SCAN_KMAX = 5                      # spgemm.hip


def out_degrees(a):
    return np.diff(a.rowptr.astype(I64))


def hub_set(a):
    """H as a list of vertex ids, H[0] the top hub."""
    deg = out_degrees(a)
    top = int(deg.max())
    q = np.nonzero(deg >= -(-top // DEG_DEN))[0]
    order = np.lexsort((q, -deg[q]))                         # degree descending, id ascending
    return [int(v) for v in q[order][:SET_MAX]]


def union_rows(a, hubs):
    """The union of out(h) over `hubs`, each row once, ascending."""
    return np.unique(np.concatenate([a.row(int(h)).astype(I64) for h in hubs]))


def shares(a, hubs):
    """(entries of A' in the rows out(H[0]), entries in the union's rows outside out(H[0])) / all entries"""
    indeg = np.bincount(a.colidx[:a.nnz].astype(I64), minlength=a.ncols)
    first = int(indeg[a.row(int(hubs[0])).astype(I64)].sum())
    both = int(indeg[union_rows(a, hubs)].sum())
    return first / a.nnz, (both - first) / a.nnz


def levels(a):
    """Reduced plans the snapshot keeps: 0, 1 (the top hub's) or 2 (the hub set's as well)."""
    hubs = hub_set(a)
    indeg = np.bincount(a.colidx[:a.nnz].astype(I64), minlength=a.ncols)
    first = int(indeg[a.row(hubs[0]).astype(I64)].sum())
    if first * HUB_SHARE_DEN < a.nnz or first >= a.nnz:
        return 0
    if len(hubs) < 2:
        return 1
    both = int(indeg[union_rows(a, hubs)].sum())
    return 2 if (both - first) * SET_SHARE_DEN >= a.nnz and both < a.nnz else 1


def hub_mask(a, at, hubs):
    """mask[u] bit i: (u, hubs[i]) is an entry of a (`at` = its transpose)."""
    mask = np.zeros(a.nrows, dtype=np.uint64)
    for i, h in enumerate(hubs):
        mask[at.row(int(h)).astype(I64)] |= np.uint64(1 << i)
    return mask


def tiers(a, at, src, hubs):
    """Per source: 2 when it reaches every hub of `hubs` in exactly two hops (tier A), 1 when it reaches hubs[0] but not all
    (tier B), 0 otherwise (weak)."""
    mask = hub_mask(a, at, hubs)
    full = np.uint64((1 << len(hubs)) - 1)
    out = np.zeros(len(src), dtype=I64)
    for k, s in enumerate(src):
        got = np.bitwise_or.reduce(mask[a.row(int(s)).astype(I64)], initial=np.uint64(0))
        out[k] = 2 if got == full else 1 if got & np.uint64(1) else 0
    return out


def tiered_passes(a, at, src, pass_rows, hubs=None):
    """(passes, passes under xp_hub_rows, passes under xp_hub_set, passes of class rows under xp_hub_set, live sources) of a
    whole-frontier call as expand_count_scan cuts it: the live sources tier A, tier B, weak (stable), the degree-one sources
    classed by their target — a class of m sources is one row of scale 2^k for every set bit k < kmax of m and m >> kmax rows of
    scale 2^kmax, kmax the value that gives the fewest passes — and every group cut into passes of pass_rows rows.  A group lists
    its rows in live order: tier A first, then tier B.  A pass of tier-A rows only runs under the second plan, one of strong rows
    only under a reduced plan.  With one reduced plan (`levels(a) == 1`) pass hubs=hub_set(a)[:1]: tier A is then every strong row."""
    hubs = hub_set(a) if hubs is None else hubs
    deg = out_degrees(a)[src.astype(I64)]
    live = src[deg > 0].astype(I64)
    tier = tiers(a, at, live, hubs)
    one = deg[deg > 0] == 1
    target = np.array([int(a.row(int(s))[0]) for s in live[one]], dtype=I64)
    _, first, m = np.unique(target, return_index=True, return_counts=True)
    class_tier = tier[one][first]
    nplain = int((~one).sum())
    bits = [int(((m >> k) & 1).sum()) for k in range(SCAN_KMAX + 1)]
    top = [int((m >> k).sum()) for k in range(SCAN_KMAX + 1)]
    rows_of = lambda kmax: [(0 if k else nplain) + (bits[k] if k < kmax else top[k]) for k in range(kmax + 1)]
    passes_of = lambda kmax: sum(-(-r // pass_rows) for r in rows_of(kmax))
    kmax = min(range(SCAN_KMAX + 1), key=lambda k: (passes_of(k), k))
    total = strong = deep = deep_scaled = 0
    for k, rows in enumerate(rows_of(kmax)):
        n_of = lambda t: (0 if k else int(((tier == t) & ~one).sum())) + int(
            (((m[class_tier == t] >> k) & 1) if k < kmax else (m[class_tier == t] >> kmax)).sum())
        n_a, n_b = n_of(2), n_of(1)
        for first_row in range(0, rows, pass_rows):
            end = min(first_row + pass_rows, rows)
            total += 1
            if end <= n_a:
                deep += 1
                deep_scaled += 1 if k else 0
            if end <= n_a + n_b:
                strong += 1
    return total, strong, deep, deep_scaled, len(live)
