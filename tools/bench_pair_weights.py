"""Times what feeds fgpu_msf / fgpu_sssp: the algorithms' weighted pair matrix (fgpu_pair_weights).

  python tools/bench_pair_weights.py host 18 20 [--pkg-root DIR] [--reps 3]
      algo_msf and algo_sp_paths through the host layer on the R-MAT graph of each scale, loaded with bulk_insert_edges, a
      hashed weight on every relationship.  The C API is called with numpy arrays (a 16 M-entry dict would time Python).
      --pkg-root: import falkordb_amd from another checkout (the parent commit, built), same process layout and inputs; the
      digest of the results is printed so that two runs can be compared.
  python tools/bench_pair_weights.py bare 22 [--reps 5]
      the bare call on the tensor fgpu_edges_build makes of the raw R-MAT tuples (repeated pairs = multi-edges), under OUT and
      OUT|IN with a full attribute list, kernels split by the fgpu_prof_* hooks; in the same run fgpu_edges_build of the same
      tuples, one fgpu_msf and one fgpu_sssp.

Wall-clock medians after one warm-up call (time.perf_counter around calls that return with their results on the host); the
kernel split is HIP events.  One JSON line per measurement."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights_of(ids):
    """1/8 .. 125: a hash of the id, so that neighbouring ids do not weigh alike"""
    return ((ids * np.uint64(2654435761)) % np.uint64(1000) + np.uint64(1)).astype(np.float64) / 8.0


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out, r


def host_leg(scales, reps):
    import oracle
    from falkordb_amd import host
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    L = host.load()
    hc = host.Context(0)
    for scale in scales:
        u, v = oracle.rmat_edges(scale)
        ids = np.arange(len(u), dtype=np.uint64)
        w = weights_of(ids)
        g = host.Graph(hc, 1 << scale)
        t = g.add_type("KNOWS")
        g.bulk_insert_edges(t, u, v, ids)
        src = int(np.bincount(u.astype(np.int64), minlength=1 << scale).argmax())
        deg_in = np.bincount(v.astype(np.int64), minlength=1 << scale)
        deg_in[src] = 0
        tgt = int(deg_in.argmax())

        def take(p, n, dtype=np.uint64):
            a = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype)
            L.fh_free(p)
            return a

        def msf():
            nt = C.c_uint64()
            noff, nodes, eoff, edges = u64p(), u64p(), u64p(), u64p()
            host._ck(L.fh_algo_msf(g.h, b"", b"", C.c_int(0), ids.ctypes.data_as(u64p), w.ctypes.data_as(f64p), C.c_uint64(len(ids)),
                                   C.byref(nt), C.byref(noff), C.byref(nodes), C.byref(eoff), C.byref(edges)))
            no, eo = take(noff, nt.value + 1), take(eoff, nt.value + 1)
            return [no, take(nodes, int(no[-1])), eo, take(edges, int(eo[-1]))]

        def sp():
            found, nn = C.c_int(), C.c_uint64()
            nodes, edges = u64p(), u64p()
            weight, cost = C.c_double(), C.c_double()
            host._ck(L.fh_algo_sp_paths(g.h, C.c_uint64(src), C.c_uint64(tgt), b"", C.c_int(0), ids.ctypes.data_as(u64p),
                                        w.ctypes.data_as(f64p), C.c_uint64(len(ids)), None, None, C.c_uint64(0), C.byref(found),
                                        C.byref(nodes), C.byref(nn), C.byref(edges), C.byref(weight), C.byref(cost)))
            return [take(nodes, nn.value), take(edges, max(nn.value, 1) - 1), np.array([found.value, weight.value])]

        for name, fn in (("algo_msf", msf), ("algo_sp_paths", sp)):
            med, all_ms, res = timed(fn, reps)
            digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in res)).hexdigest()[:16]
            row = {"leg": "host", "call": name, "scale": scale, "relationships": len(ids), "median_ms": round(med, 2),
                   "all_ms": [round(x, 2) for x in all_ms], "result_sha16": digest}
            if hasattr(g, "pair_stats"):
                row["pair_stats"] = g.pair_stats()
            print(json.dumps(row), flush=True)
        del g
    hc.close()


def bare_leg(scale, reps):
    import oracle
    from falkordb_amd import engine
    ctx = engine.Context(0)
    n = 1 << scale
    u, v = oracle.rmat_edges(scale)
    ids = np.arange(len(u), dtype=np.uint64)
    w = weights_of(ids)
    keep = {}

    def build():
        keep["t"] = engine.edges_build(ctx, n, n, u, v, ids)
        return keep["t"]

    med, all_ms, (fwd, bwd, mk, mo, mi) = timed(build, max(reps // 2, 1))
    print(json.dumps({"leg": "bare", "call": "fgpu_edges_build", "scale": scale, "tuples": len(u), "multi_pairs": len(mk),
                      "median_ms": round(med, 2), "all_ms": [round(x, 2) for x in all_ms]}), flush=True)
    multi = ctx.multi_new(mk, mo, mi)
    mats = {}
    for name, kw in (("OUT", dict(out=True)), ("OUT|IN", dict(out=True, inc=True))):
        def run():
            return ctx.pair_weights([fwd], None, None, [multi], attr_ids=ids, attr_vals=w, missing=1.0, **kw)
        med, all_ms, (W, K, st) = timed(run, reps)
        ctx.prof_enable(True)
        run()
        prof = {p["kernel"]: round(p["ms"], 3) for p in ctx.prof_read() if p["ms"] > 0}
        ctx.prof_enable(False)
        mats[name] = W
        print(json.dumps({"leg": "bare", "call": "fgpu_pair_weights " + name, "scale": scale, "median_ms": round(med, 2),
                          "all_ms": [round(x, 2) for x in all_ms], "stats": st, "prof_ms": prof}), flush=True)
    med, all_ms, r = timed(lambda: engine.msf(ctx, mats["OUT|IN"]), reps)
    print(json.dumps({"leg": "bare", "call": "fgpu_msf", "scale": scale, "median_ms": round(med, 2), "forest_edges": len(r[1])}), flush=True)
    src = int(np.bincount(u.astype(np.int64), minlength=n).argmax())
    med, all_ms, r = timed(lambda: engine.sssp(ctx, mats["OUT"], src), reps)
    print(json.dumps({"leg": "bare", "call": "fgpu_sssp", "scale": scale, "median_ms": round(med, 2),
                      "reached": int(np.isfinite(r[0]).sum())}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["host", "bare"])
    ap.add_argument("scales", type=int, nargs="+")
    ap.add_argument("--pkg-root", default=ROOT)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)            # (oracle, for the tuples)
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    if a.leg == "host":
        host_leg(a.scales, a.reps)
    else:
        bare_leg(a.scales[0], a.reps)
