#!/usr/bin/env python3
"""Times fgpu_vecidx_knn (the search behind db.idx.vector.queryNodes) on one GPU, outside bench.py.

Store: 2^20 vectors at dim 128 and dim 1024, euclidean, uniform [-1, 1) f32 from a seed.  knn with k = 10 at nq = 1, 16 and
1024: the median of repeated warm calls by a host clock (at least --reps of them and a timed window of --window seconds; the
call ends in a device synchronise and includes the read-back of the result), then in a second pass, with the context's event
profiler on, the time inside scoring, selection, the FP64 distances and the read-back (10 calls, averaged).  Each figure is printed beside what it is held against: count * dim * 4 bytes over the 8 TB/s HBM
peak for nq <= 16, 2 * nq * count * dim flops over the 157 TF f32-MFMA peak for nq = 1024, and the same search in numpy on
the CPU threads of the machine as context.  One JSON line per shape; --out also writes them to a file.

    python tools/bench_vecidx.py [--count-log2 20] [--dims 128,1024] [--nqs 1,16,1024] [--reps 20] [--window 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from falkordb_amd import engine  # noqa: E402

HBM_PEAK = 8.0e12    # bytes / s
MFMA_F32_PEAK = 157.3e12   # flop / s
PROF_CALLS = 10   # calls the profiled pass averages over


def numpy_knn(x, xn, q, k):
    """the same exhaustive search on the CPU: one f32 GEMM, argpartition, exact re-scoring of the k survivors left out"""
    key = (q * q).sum(1)[:, None] + xn[None, :] - 2.0 * (q @ x.T)
    part = np.argpartition(key, k - 1, axis=1)[:, :k]
    return np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, 1), axis=1), 1)


def median_ms(call, reps, window=0.0):
    """(median, min, calls): at least `reps` calls, and as many more as fill `window` seconds"""
    t = []
    t_start = time.perf_counter()
    while len(t) < reps or (time.perf_counter() - t_start < window and len(t) < 20000):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), len(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count-log2", type=int, default=20)
    ap.add_argument("--dims", default="128,1024")
    ap.add_argument("--nqs", default="1,16,1024")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20, help="timed calls per shape at least")
    ap.add_argument("--window", type=float, default=1.0, help="... and as many more as fill this many seconds")
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    count = 1 << a.count_log2
    ctx = engine.Context(0)
    lines = []
    for dim in [int(d) for d in a.dims.split(",")]:
        rng = np.random.default_rng(dim)
        idx = engine.VecIndex(ctx, dim, "euclidean")
        x = np.empty((count, dim), dtype=np.float32)
        step = max(1, (64 << 20) // (dim * 4))
        for lo in range(0, count, step):   # generated and uploaded in pieces of 64 MiB
            hi = min(count, lo + step)
            x[lo:hi] = rng.uniform(-1, 1, size=(hi - lo, dim)).astype(np.float32)
            idx.set(np.arange(lo, hi, dtype=np.uint64), x[lo:hi])
        xn = (x * x).sum(1)
        per_query = {}
        for nq in [int(n) for n in a.nqs.split(",")]:
            q = rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)
            ids, _, st = idx.knn(q, a.k, stats=True)   # warm-up of this shape, and the counters
            med, best, calls = median_ms(lambda: idx.knn(q, a.k), a.reps, a.window)
            ctx.prof_enable(True)
            ctx.prof_read()
            for _ in range(PROF_CALLS):
                idx.knn(q, a.k)
            parts = {}
            for rec in ctx.prof_read():
                parts[rec["kernel"]] = parts.get(rec["kernel"], 0.0) + rec["ms"] / PROF_CALLS
            ctx.prof_enable(False)
            pick = np.unique(np.linspace(0, nq - 1, min(nq, 64)).astype(np.int64))   # spread over every chunk of the batch
            cq = q[pick]
            cpu_ms, _, _ = median_ms(lambda: numpy_knn(x, xn, cq, a.k), a.cpu_reps)
            cpu_ids = numpy_knn(x, xn, cq, a.k)
            agree = float(np.mean([len(set(ids[pick[r]].tolist()) & set(cpu_ids[r].tolist())) / a.k for r in range(len(cq))]))
            store_bytes = count * dim * 4
            flops = 2.0 * nq * count * dim
            floor_ms = max(store_bytes / HBM_PEAK, flops / MFMA_F32_PEAK) * 1e3
            per_query[nq] = med / nq
            line = {
                "bench": "vecidx_knn", "count": count, "dim": dim, "metric": "euclidean", "k": a.k, "nq": nq,
                "call_ms_median": round(med, 4), "call_ms_min": round(best, 4), "timed_calls": calls, "per_query_ms": round(med / nq, 5),
                "score_ms": round(parts.get("vec_score", 0.0), 4), "select_ms": round(parts.get("vec_select", 0.0), 4),
                "dist_ms": round(parts.get("vec_dist", 0.0), 4), "readback_ms": round(parts.get("vec_readback", 0.0), 4),
                "scoring_launches": st[0], "query_tiles": st[1], "store_bytes_read": st[2],
                "hbm_floor_ms": round(store_bytes / HBM_PEAK * 1e3, 4), "mfma_floor_ms": round(flops / MFMA_F32_PEAK * 1e3, 4),
                "bound": "hbm" if store_bytes / HBM_PEAK >= flops / MFMA_F32_PEAK else "mfma",
                "score_share_of_floor": round(floor_ms / parts["vec_score"], 4) if parts.get("vec_score") else None,
                "score_gbps": round(st[2] / parts["vec_score"] / 1e6, 1) if parts.get("vec_score") else None,
                "score_tflops": round(flops / parts["vec_score"] / 1e9, 2) if parts.get("vec_score") else None,
                "numpy_queries": len(cq), "numpy_ms_per_query": round(cpu_ms / len(cq), 3),
                "numpy_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None, "top_k_overlap_with_numpy": round(agree, 4),
            }
            lines.append(line)
            print(json.dumps(line), flush=True)
        if 1 in per_query and 1024 in per_query:
            line = {"bench": "vecidx_knn_batching", "dim": dim, "per_query_ms_nq1": round(per_query[1], 5),
                    "per_query_ms_nq1024": round(per_query[1024], 5), "ratio": round(per_query[1] / per_query[1024], 2)}
            lines.append(line)
            print(json.dumps(line), flush=True)
        idx.free()
        del x, xn
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
