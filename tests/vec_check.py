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
    """the f32 key of fgpu.h for euclidean and ip, with every operation rounded to f32 one by one — the fmaf chain itself
    only where every product and partial sum is exact in f32 (the integer generators)"""
    q = np.asarray(q, dtype=np.float32).reshape(1, -1)
    x = np.asarray(x, dtype=np.float32)

    def chain(a, b):
        acc = np.zeros(max(a.shape[0], b.shape[0]), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (acc + a[:, i] * b[:, i]).astype(np.float32)
        return acc
    s = chain(q, x)
    if metric == "ip":
        return -s
    assert metric == "euclidean"
    t = (chain(q, q) + chain(x, x)).astype(np.float32)
    return (t - np.float32(2.0) * s).astype(np.float32)


def topk(keys, ids, k):
    """positions of the min(k, n) entries of smallest (key, id), in that order"""
    return np.lexsort((np.asarray(ids), np.asarray(keys)))[:min(int(k), len(keys))]


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
    """integer components in [-8, 8]: with dim <= 130 every f32 operation of the euclidean and ip keys is exact"""
    return rng.integers(-8, 9, size=(count, dim)).astype(np.float32)


def float_store(count, dim, nq, seed=7):
    """(store, queries) uniform in [-1, 1) as f32, from one generator"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(count, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)
    return x, q


def scattered_ids(rng, count):
    """distinct ids that are neither the slots nor in order"""
    return rng.permutation(3 * count + 7)[:count].astype(np.uint64)
