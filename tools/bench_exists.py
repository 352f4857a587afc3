"""Times the pattern predicate: fgpu_expand_exists beside the two ways the same bits could be had before it, and
SemiApplyOp::filter_batch with the existence tier on and off.

  python tools/bench_exists.py device 22 [--batches 8] [--reps 5] [--out FILE.jsonl]
      Batches of 1024 :P source rows (bench.py's label) on the R-MAT graph of the scale, chains of 1, 2 and 3 hops, over clean
      layers, over bench.py's dirty layers (0.1 % of the entries tombstoned, as many added) and over a heavier tombstone layer
      (5 %).  Per chain: fgpu_expand_exists; fgpu_expand_pairs32 plus collecting the rows that occur; fgpu_expand_count; and
      fgpu_expand_count of the chain one hop shorter, which is what the last step of the predicate follows.  The answers of the
      first two are compared.  Then, profiler on in a pass of its own, the kernels of the last step.
  python tools/bench_exists.py host 20 [--batches 8] [--reps 5]
      The same batches through SemiApplyOp::filter_batch on a host graph loaded with bulk_insert_edges, device_exists on and
      off (the collect tier: the reference's own method), one type, 1 to 3 hops; the operator's own time (fh_last_op_ns).

Every figure is a wall-clock time around a call that returns with its result on the host (the calls synchronise), after one
warm-up pass over every batch; the variants alternate inside each repetition.  Reported: the median over batches x reps, the
quartiles and the extremes.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def alternate(variants, batches, reps):
    """{name: [ms]}: one warm-up pass, then reps passes with the variants alternating on every batch."""
    for b in batches:
        for fn in variants.values():
            fn(b)
    ms = {name: [] for name in variants}
    for _ in range(reps):
        for b in batches:
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn(b)
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def pairs32_rows(ctx, src, m, dp, dm):
    """fgpu_expand_pairs32 (16-bit row indices, 32-bit destinations: what CondTraverseOp::expand_batch takes) and the rows
    that occur — the way to these bits before fgpu_expand_exists."""
    import ctypes as C
    from falkordb_amd import engine
    from falkordb_amd._ffi import check
    src = np.ascontiguousarray(src, dtype=np.uint64)
    am = engine._hop_arrays(m)
    adp = engine._hop_arrays(dp) if dp is not None else None
    adm = engine._hop_arrays(dm) if dm is not None else None
    prow, pdest = C.c_void_p(), C.POINTER(C.c_uint32)()
    n, flops = C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand_pairs32(ctx._h, src.ctypes.data_as(C.POINTER(C.c_uint64)), len(src), am, adp, adm, len(m), None, None,
                                      16, C.byref(prow), C.byref(pdest), C.byref(n), C.byref(flops)))
    if n.value == 0:
        return np.zeros(0, dtype=np.uint16)
    rows = np.unique(np.ctypeslib.as_array(C.cast(prow, C.POINTER(C.c_uint16)), shape=(n.value,)))
    ctx.lib.fgpu_free(ctx._h, prow)
    ctx.lib.fgpu_free(ctx._h, pdest)
    return rows


def device_leg(scale, nbatches, reps, out):
    import bench
    from falkordb_amd import engine
    ctx = engine.Context(0)
    A, dp, dm, _ = bench.khop_inputs(ctx, scale, 16)
    dm5 = A.sample(0x70B5 + scale, 20)                       # a twentieth of the entries tombstoned, unfolded
    src = bench.p_label_sources(A.nrows)
    batches = [src[i * 1024:(i + 1) * 1024] for i in range(nbatches)]
    layer_sets = {"clean": (None, None), "dirty 0.1 %": (dp, dm), "tombstones 5 %": (None, dm5)}
    for hops in (1, 2, 3):
        for lname, (p, m_) in layer_sets.items():
            M = [A] * hops
            P = [p] * hops if p is not None else None
            D = [m_] * hops if m_ is not None else None
            stats_sum = np.zeros(4, dtype=np.int64)
            same = True
            for b in batches:
                got, _, st = engine.expand_exists(ctx, b, M, P, D)
                want = np.zeros(len(b), dtype=bool)
                want[pairs32_rows(ctx, b, M, P, D).astype(np.int64)] = True
                same = same and bool(np.array_equal(got, want))
                stats_sum += np.array(st, dtype=np.int64)

            def pairs_rows(b):
                return pairs32_rows(ctx, b, M, P, D)

            variants = {
                "exists": lambda b: engine.expand_exists(ctx, b, M, P, D),
                "pairs + rows": pairs_rows,
                "count": lambda b: engine.expand_count(ctx, b, M, P, D),
            }
            if hops > 1:
                variants["count, chain before the last hop"] = lambda b: engine.expand_count(
                    ctx, b, M[:-1], P[:-1] if P else None, D[:-1] if D else None)
            ms = alternate(variants, batches, reps)
            rec = {"leg": "device", "scale": scale, "hops": hops, "layers": lname, "rows_per_batch": 1024, "batches": nbatches,
                   "answers_equal": same, "rows_matched": int(stats_sum[0]), "rows_undecided": int(stats_sum[1]),
                   "undecided_share": round(float(stats_sum[1]) / (1024 * nbatches), 6),
                   "entries_read_per_batch": int(stats_sum[2] // nbatches), "bit_form_batches": int(stats_sum[3])}
            for name, v in ms.items():
                rec[name] = spread(v)
            emit(out, rec)
            # the kernels of the last step, in a pass of its own
            ctx.prof_enable(True)
            try:
                for b in batches:
                    engine.expand_exists(ctx, b, M, P, D)
                prof = [p_ for p_ in ctx.prof_read()]
            finally:
                ctx.prof_enable(False)
            tot = sum(p_["ms"] for p_ in prof)
            last = {p_["kernel"]: round(p_["ms"] / nbatches, 4) for p_ in prof if p_["kernel"].startswith("exists_")}
            emit(out, {"leg": "device kernels", "scale": scale, "hops": hops, "layers": lname,
                       "all_kernels_ms_per_batch": round(tot / nbatches, 4), "last_step_ms_per_batch": last})
    ctx.close()


def host_leg(scale, nbatches, reps, out):
    import bench
    import oracle
    from falkordb_amd import host
    L = host.load()
    hc = host.Context(0)
    u, v = oracle.rmat_edges(scale)
    g = host.Graph(hc, 1 << scale)
    t = g.add_type("KNOWS")
    g.bulk_insert_edges(t, u, v, np.arange(len(u), dtype=np.uint64))
    src = bench.p_label_sources(1 << scale)
    batches = [src[i * 1024:(i + 1) * 1024].tolist() for i in range(nbatches)]
    for hops in (1, 2, 3):
        spec = host.cond_spec(hops=[(["KNOWS"], [])] + [([], [])] * (hops - 1))
        op_ms = {"device_exists on": [], "device_exists off": []}

        def run(b, on):
            got = g.semi_apply(spec, b, device_exists=on)
            op_ms["device_exists on" if on else "device_exists off"].append(L.fh_last_op_ns() / 1e6)
            return got

        same = all(run(b, True)[0] == run(b, False)[0] for b in batches)
        tiers = (run(batches[0], True)[1], run(batches[0], False)[1])
        for k_ in op_ms:
            op_ms[k_].clear()
        ms = alternate({"device_exists on": lambda b: run(b, True), "device_exists off": lambda b: run(b, False)}, batches, reps)
        warm = len(batches)                                 # the warm-up pass of alternate() is dropped from the operator times
        rec = {"leg": "host", "scale": scale, "hops": hops, "rows_per_batch": 1024, "batches": nbatches, "answers_equal": same,
               "tiers": tiers}
        for name in ms:
            rec[name] = {"call": spread(ms[name]), "operator": spread(op_ms[name][warm:])}
        emit(out, rec)
    hc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["device", "host"])
    ap.add_argument("scales", type=int, nargs="+")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for s in a.scales:
        (device_leg if a.leg == "device" else host_leg)(s, a.batches, a.reps, out)


if __name__ == "__main__":
    main()
