"""The checker of the vector index tests: numpy, FP64, no engine code.

D(q, x) is fgpu_vecidx_knn's reported distance (include/fgpu.h, after the reference's runtime/vec_distance.rs); keys64 is the
FP64 value of the quantity the device selects by in f32; band_ok is the rule a float result is held to, given the f32
rounding bound of that key."""
import numpy as np

METRICS = ("euclidean", "cosine", "ip")
U = 2.0 ** -24   # unit roundoff of f32


def _rows(x):
    x = np.asarray(x, dtype=np.float32)
    return (x.reshape(1, -1) if x.ndim == 1 else x).astype(np.float64)


def _dot(a, b):
    """sum_i a[:, i] * b[:, i] accumulated in index order"""
    acc = np.zeros(max(a.shape[0], b.shape[0]), dtype=np.float64)
    for i in range(a.shape[1]):
        acc = acc + a[:, i] * b[:, i]
    return acc


def dist(metric, q, x):
    """D(q, x[r]) for every row r of x (one float64 per row); q is one vector"""
    q, x = _rows(q), _rows(x)
    assert q.shape[0] == 1 and q.shape[1] == x.shape[1]
    if metric == "euclidean":
        d = q - x
        return np.sqrt(_dot(d, d))
    if metric == "ip":
        return -_dot(q, x)
    assert metric == "cosine"
    qq, xx = _dot(q, q), _dot(x, x)
    den = np.sqrt(qq) * np.sqrt(xx)
    zero = (qq == 0.0) | (xx == 0.0)
    return np.where(zero, 1.0, 1.0 - _dot(q, x) / np.where(zero, 1.0, den))


def keys64(metric, q, x):
    """the selection key in FP64: ||q||^2 + ||x||^2 - 2 q.x, -q.x, or the cosine distance"""
    q, x = _rows(q), _rows(x)
    if metric == "euclidean":
        return (_dot(q, q) + _dot(x, x)) - 2.0 * _dot(q, x)
    return dist(metric, q, x)


def keys32(metric, q, x):
    """the f32 key of fgpu.h, with every operation rounded to f32 one by one — the fmaf chain itself only where every product
    and partial sum is exact in f32 (the integer generators).  Cosine: the three chains S, nq and nx, then
    fl(1 - fl(S / fl(fl(sqrt nq) * fl(sqrt nx)))) (numpy's float32 sqrt, product, quotient and difference are each correctly
    rounded), and 1.0 where nq or nx is 0."""
    q = np.asarray(q, dtype=np.float32).reshape(1, -1)
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x

    def chain(a, b):
        acc = np.zeros(max(a.shape[0], b.shape[0]), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (acc + a[:, i] * b[:, i]).astype(np.float32)
        return acc
    s = chain(q, x)
    if metric == "ip":
        return -s
    nq, nx = chain(q, q), chain(x, x)
    if metric == "cosine":
        zero = (nq == 0) | (nx == 0)
        den = (np.sqrt(nq).astype(np.float32) * np.sqrt(nx).astype(np.float32)).astype(np.float32)
        with np.errstate(all="ignore"):   # (a denominator that underflowed: the key is the inf or NaN the division gives)
            ratio = (s / np.where(zero, np.float32(1.0), den)).astype(np.float32)
            key = (np.float32(1.0) - ratio).astype(np.float32)
        return np.where(zero, np.float32(1.0), key).astype(np.float32)
    assert metric == "euclidean"
    t = (nq + nx).astype(np.float32)
    return (t - np.float32(2.0) * s).astype(np.float32)


def topk(keys, ids, k):
    """positions of the min(k, n) entries of smallest (key, id), in that order"""
    return np.lexsort((np.asarray(ids), np.asarray(keys)))[:min(int(k), len(keys))]


def expected_ties(k, keys, ids=None):
    """stats[3] of one query: t = the entries whose key equals the kk-th smallest key, when t exceeds the places left after
    the strictly smaller keys (the id order had to decide), otherwise 0.  The ids do not change the count."""
    keys = np.asarray(keys)
    kk = min(int(k), len(keys))
    if kk == 0:
        return 0
    kth = np.partition(keys, kk - 1)[kk - 1]
    t, less = int(np.sum(keys == kth)), int(np.sum(keys < kth))
    return t if t > kk - less else 0


def batch_keys(metric, queries, x):
    """keys64 of a whole batch, float64[nq, count], by one matrix product — for INTEGER inputs only (int_store), where every
    product and sum is exact in FP64 whatever the order, so this is keys64 bit for bit; euclidean and ip"""
    q = np.asarray(queries, dtype=np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    q = q.reshape(1, -1) if q.ndim == 1 else q
    assert np.all(q == np.round(q)) and np.all(x == np.round(x)), "batch_keys is exact for integer components only"
    s = q @ x.T
    if metric == "ip":
        return -s
    assert metric == "euclidean"
    return ((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :]) - 2.0 * s


def batch_dist(metric, keys):
    """D from the integer-exact keys of batch_keys: the euclidean key is the squared distance, the ip key the distance"""
    return np.sqrt(keys) if metric == "euclidean" else keys


def batch_topk(keys, ids, k):
    """topk for every row of keys[nq, count]: (positions int64[nq, kk] in (key, id) order, the sum of expected_ties).  A
    partition finds each row's kk-th key; only the entries at that key are picked by id.  Ids already ascending cost no
    gather."""
    keys, ids = np.asarray(keys), np.asarray(ids)
    nq, n = keys.shape
    kk = min(int(k), n)
    in_order = n < 2 or bool(np.all(ids[1:] > ids[:-1]))
    by_id = np.arange(n) if in_order else np.argsort(ids, kind="stable")
    out = np.zeros((nq, kk), dtype=np.int64)
    ties = 0
    for r in range(nq):
        row = keys[r] if in_order else keys[r, by_id]   # in id order: a stable sort by key is then the (key, id) order
        if kk == n:
            out[r] = by_id[np.argsort(row, kind="stable")]
            continue
        kth = np.partition(row, kk - 1)[kk - 1]
        less, tie = np.flatnonzero(row < kth), np.flatnonzero(row == kth)
        if len(tie) > kk - len(less):
            ties += len(tie)
        sure = less[np.argsort(row[less], kind="stable")]
        out[r] = by_id[np.concatenate([sure, tie[:kk - len(less)]])]
    return out, ties


def check_batch(metric, ids, x, queries, k, got_ids, got_d, tol, rows_per_block=None):
    """The vectorised form of the GPU tests' check_exact, for integer inputs: got_ids[nq, kk] entry for entry the top-k by
    (key, id), got_d within tol (relative above 1) of D.  Returns the sum of expected_ties over the queries.  The keys are
    made a block of queries at a time, at most 2^23 of them."""
    ids, x = np.asarray(ids), np.asarray(x, dtype=np.float32)
    queries = np.asarray(queries, dtype=np.float32)
    queries = queries.reshape(1, -1) if queries.ndim == 1 else queries
    nq, n = len(queries), len(ids)
    kk = min(int(k), n)
    assert got_ids.shape == (nq, kk) and got_d.shape == (nq, kk), (got_ids.shape, got_d.shape, (nq, kk))
    step = rows_per_block or max(1, (1 << 23) // max(n, 1))
    ties = 0
    by_id = np.argsort(ids, kind="stable")
    ids, x = ids[by_id], x[by_id]                   # the store in id order, once
    for r0 in range(0, nq, step):
        keys = batch_keys(metric, queries[r0:r0 + step], x)
        top, t = batch_topk(keys, ids, k)
        ties += t
        want_ids = ids[top]
        want_d = batch_dist(metric, np.take_along_axis(keys, top, axis=1))
        g_ids, g_d = got_ids[r0:r0 + step], got_d[r0:r0 + step]
        if not np.array_equal(g_ids, want_ids):
            r, c = np.argwhere(g_ids != want_ids)[0]
            raise AssertionError(f"query {r0 + r}, place {c}: id {g_ids[r, c]}, expected {want_ids[r, c]}")
        bad = ~(np.abs(g_d - want_d) <= tol * np.maximum(1.0, np.abs(want_d)))
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"query {r0 + r}, place {c}: distance {g_d[r, c]!r}, expected {want_d[r, c]!r}")
    return ties


def gamma(n):
    return n * U / (1.0 - n * U)


def margin(metric, q, x):
    """the f32 rounding bound m of the key, maximised over the store"""
    q, x = _rows(q), _rows(x)
    dim = x.shape[1]
    if metric == "cosine":
        return 3.0 * gamma(dim + 4)
    ab = _dot(np.abs(q), np.abs(x))
    if metric == "ip":
        return float(np.max(gamma(dim + 1) * ab))
    return float(np.max(gamma(dim + 3) * (_dot(q, q) + _dot(x, x) + 2.0 * ab)))


def band(k, keys, ids, m):
    """(the true top-k ids, B = the ids whose FP64 key lies within 2 m of the k-th)"""
    keys, ids = np.asarray(keys), np.asarray(ids)
    top = topk(keys, ids, k)
    kth = keys[top[-1]]
    return set(ids[top].tolist()), set(ids[np.abs(keys - kth) <= 2.0 * m].tolist())


def band_ok(returned_ids, k, keys, m, ids=None):
    """the returned set contains (true top-k minus B) and lies inside (true top-k plus B); ids default to the positions"""
    ids = np.arange(len(keys)) if ids is None else np.asarray(ids)
    top, b = band(k, keys, ids, m)
    got = set(np.asarray(returned_ids).tolist())
    return len(got) == len(top) and (top - b) <= got and got <= (top | b)


def int_store(rng, count, dim):
    """integer components in [-8, 8]: every f32 operation of the euclidean and ip keys is exact up to FGPU_VECIDX_DIM_MAX.
    A product is at most 64 in magnitude, so a partial sum of S, nq or nx stays within 64 * 4096 = 2^18; nq + nx within 2^19,
    2 S within 2^19 and the euclidean key within 2^20: all integers below 2^24, which f32 holds exactly."""
    return rng.integers(-8, 9, size=(count, dim)).astype(np.float32)


# (dim, count) -> the seed of cosine_case.  At dim 3 the seeds are chosen so that some query's top-10 by the f32 key is not its
# top-10 by the FP64 key (tests/test_vecidx_cpu.py pins that), so a key rounded otherwise than fgpu.h says fails the test.
COSINE_SEEDS = {(3, 255): 0, (3, 1001): 4, (5, 255): 1, (5, 1001): 1, (33, 255): 1, (33, 1001): 1}


def cosine_case(seed, count, dim, nq):
    """(store, queries, ids) of the exact cosine tests: int_store with about one stored vector in 50 all zeros (slot
    count // 2 always) and query nq // 2 all zeros.  The chains S, nq and nx are exact, so keys32 is the device's key."""
    rng = np.random.default_rng(seed)
    x, q = int_store(rng, count, dim), int_store(rng, nq, dim)
    x[rng.random(count) < 0.02] = 0.0
    x[count // 2] = 0.0
    q[nq // 2] = 0.0
    return x, q, scattered_ids(rng, count)


def parallel_case(seed, nq, families=20, members=50):
    """(store, queries, ids) at dim 3: `families` directions with integer components in [-30, 30], each stored under `members`
    integer multiples up to 60, and one stray vector; the queries are further multiples of those directions.  Components
    stay within 1800, so S, nq and nx are integers below 2^24 and exact, and keys32 is the device's cosine key.  In real
    arithmetic a query's keys to one family are all equal; in f32 they fall on a few neighbouring values according to how
    each sqrt, product and quotient rounds, so the (key, id) order inside a family shows every rounding of the key."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-30, 31, size=(families, 3))
    base[~base.any(axis=1)] = 1
    mult = rng.integers(1, 61, size=(families, members))
    x = (base[:, None, :] * mult[:, :, None]).reshape(-1, 3)
    x = np.concatenate([x, rng.integers(-1800, 1801, size=(1, 3))]).astype(np.float32)
    q = (base[rng.integers(0, families, nq)] * rng.integers(1, 61, size=(nq, 1))).astype(np.float32)
    return x, q, scattered_ids(rng, len(x))


def float_store(count, dim, nq, seed=7):
    """(store, queries) uniform in [-1, 1) as f32, from one generator"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(count, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)
    return x, q


def scattered_ids(rng, count):
    """distinct ids that are neither the slots nor in order"""
    return rng.permutation(3 * count + 7)[:count].astype(np.uint64)


ID_MAX = 2 ** 32 - 2   # the largest id an index takes
# 0 and ID_MAX, each beside ids that differ from it in the top byte alone and ids that differ in the low byte alone
WIDE_FIXED = (0, 1, 0xFF, 1 << 24, 0xFF << 24, ID_MAX, ID_MAX ^ (0xFF << 24), ID_MAX ^ 0xFE)


def wide_ids(rng, count):
    """count >= 8 distinct ids over the whole range 0 .. 2^32 - 2, in no order: WIDE_FIXED, then random ids each followed by
    a copy with another top byte and a copy with another low byte, so that every byte of the id decides some comparison"""
    assert count >= len(WIDE_FIXED)
    v = rng.integers(0, ID_MAX + 1, size=count // 3 + count // 64 + 8, dtype=np.uint64)   # (some repeat: a few more)
    top = v ^ (rng.integers(1, 256, size=len(v), dtype=np.uint64) << np.uint64(24))
    low = v ^ rng.integers(1, 256, size=len(v), dtype=np.uint64)
    cand = np.concatenate([np.array(WIDE_FIXED, dtype=np.uint64), np.stack([v, top, low], axis=1).ravel()])
    cand = cand[cand <= ID_MAX]
    _, first = np.unique(cand, return_index=True)
    ids = cand[np.sort(first)][:count]           # first occurrences, in the order made: the fixed ones and whole triples
    assert len(ids) == count
    return rng.permutation(ids)
