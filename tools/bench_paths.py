"""Secondary hot-path measurements (one JSON line each; bench.py stays the BFS headline):

  merge   Delta merge (m \\ dm) U dp on RMAT-<scale> with 0.1 % pending adds + 0.1 % tombstones
          (SURVEY §8d config 5 "merge GB/s"; K6): entry-parallel kernel vs the wavefront-per-row one,
          pattern and UINT64 layers
  expand  k-hop CondTraverse core (fgpu_expand_count) on RMAT-<scale>, 1024-row batches, clean and dirty
          layers
  host    CondTraverseOp::expand_batch through the C++ host layer vs the bare fgpu_expand call

  reach   [*1..4] DISTINCT reachability (fgpu_expand_levels) with dirty layers, device fold, folded rerun
          (SURVEY §8d config 5 stand-in)

  pagerank  algo.pageRank's core (fgpu_pagerank, FP32 plus_second pull SpMV) on RMAT-<scale>: ms per iteration

  wcc     algo.WCC's core (fgpu_wcc) on RMAT-22 and RMAT-24 (or RMAT-<scale>): (A, At) and the symmetrised A with At = NULL,
          wcc_mode 1 (Afforest, sampling + skip) and 2 (one full link pass); median of 10 synchronised calls, the stats,
          and the full-pass bound (4 nnz(A) + 4 (n + 1) bytes at 8 TB/s)

  betweenness  algo.betweenness' core (fgpu_betweenness) on RMAT-22 and RMAT-24 (or RMAT-<scale>): 16 sources of seed 0 (ids
          0..15, R-MAT's hubs), 16 and 256 LCG-drawn sources (samplingSeed 10), each under bc_direction 0 / 1 / 2; median of
          10 synchronised calls, the stats, fgpu_bfs once per source as a yardstick, and the bound (per batch: the CSR read
          forward and backward, 2 (4 nnz + 4 (n + 1)) bytes, plus the per-(vertex, source) state written and read,
          2 n B (8 + 8 + 4) bytes, at 8 TB/s)

  cdlp    algo.labelPropagation's core (fgpu_cdlp) on the symmetrised RMAT-22 and RMAT-24 (or RMAT-<scale>), itermax = 10;
          median of 10 synchronised calls after 2 warm-ups, the stats, ms per iteration, the bytes an iteration must move
          (4 nnz column ids + 4 nnz gathered labels + 8 n for the two label arrays) as a share of 8 TB/s, and fgpu_pagerank's
          time per iteration on the same matrix (the same columns read, one 4-byte gather per entry: the nearest yardstick)

  harmonic  algo.HarmonicCentrality's core (fgpu_harmonic, HyperBall over 1 KiB sketches) on the RMAT-22 adjacency (or
          RMAT-<scale>): median of 5 synchronised calls after 1 warm-up, the stats, the iterations, ms per iteration (the call
          less the fixed part — the same call on an empty matrix of that size: clearing 2 n KiB, the init pass, the copy-out —
          over the iterations), and the gathered bytes per second: entries of the recomputed rows x 1 KiB, and the sketches
          the kernels actually loaded x 1 KiB (entries whose column did not change are not loaded), against the 5.5 TB/s
          measured for register gathers of random 1152-byte rows

  sssp    algo.SPpaths' core (fgpu_sssp, near / far delta-stepping) on RMAT-22 (or RMAT-<scale>) with hashed weights, integers
          1..100 and uniform doubles in [0, 1), from the vertex with the most out-entries: median of 3 synchronised calls, the
          stats, the reached vertices, the bucket width, and one fgpu_bfs and one full-pass vxm over the same pattern;
          sssp_sweep = the same under nine bucket widths around the derived one

  asp     allShortestPaths' core (fgpu_shortest_dag, bidirectional level-synchronous search + the DAG sweeps) on RMAT-22 (or
          RMAT-<scale>), directed and symmetrised (A + A'), 64 (src, dst) pairs drawn at a fixed seed among the vertices with
          an out- and an in-entry: per pair L, the DAG pairs, the eight stats and the ms per call under spdag_sides 0 (two-sided)
          and 1 (forward only), median / min / max of 5 synchronised calls after 1 warm-up, and one fgpu_bfs (levels only) from
          the same src; then one summary line per graph with the medians over the pairs and the ratios

  asp_batch  fgpu_shortest_dag_batch against a loop of fgpu_shortest_dag, in ONE process, on the graph and the 64 seeded pairs of
          the asp leg, directed and symmetrised: (a) the loop of 64 single calls, (b) one batch of the same 64, (c) one batch of
          1024 seeded pairs at slots = 0.  Median / min / max of 5 after 1 warm-up, ms per query, the entries scanned (stats [4]
          and [5] summed), and that (b) returned what (a) did; with the host operator's batch against its per-row loop on the
          host leg's graph (RMAT-18, one type, 64 rows, fh_last_op_ns)

  shortest_path  fgpu_shortest_path_batch (shortestPath()'s one path per query) on the graph and the seeded pairs of the asp_batch
          leg, directed and symmetrised, in ONE process: (a) a loop of 64 calls of one query, (b) one call of the same 64, (c) one
          of the 1024 pairs at slots = 0, (d) / (e) fgpu_shortest_dag_batch on the pairs of (b) / (c) as the yardstick.  Median /
          min / max of 5 after 1 warm-up, ms per query, the entries walked, and that (b) returned what (a) did; with the host
          function's batch against its eval_row loop on the host leg's graph (RMAT-18, one type, 64 rows, fh_last_op_ns)

  hops    the hop-bounded table behind algo.SPpaths' enumeration shapes (fgpu_sssp_hops) on RMAT-22 (or RMAT-<scale>)
          TRANSPOSED, with the hashed integer weights of the sssp leg, from the vertex with the most in-entries of the graph
          (= most out-entries of the transpose): max_hops 3 and 6 into a pinned table, median of 3 synchronised calls, the
          stats, the table's bytes and the time of a pinned device-to-host copy of that many bytes on its own (so the device
          part is the call less that copy); in the same run one fgpu_sssp (distances only), one fgpu_bfs and one fgpu_sssp_hops
          from a vertex without entries (the fixed part: weight pass, row copies, launches, DMA).  Then, on the host leg's
          graph (RMAT-18, one type), one algo_sp_paths_rows call (maxLen 4, pathCount 0) with prune on and off: ms and the
          successors examined, the unpruned walk under a budget of 300 000 successors

  load    the host layer's graph load: Graph::create_edges (edge by edge through the pending logs) against
          Graph::bulk_insert_edges (one fgpu_edges_build, the result adopted as the tensor's base) on twin graphs of the distinct
          RMAT-18 and RMAT-20 edges, both in this process, alternating, a host clock around load + commit (both end in a sync),
          one warm-up, median of 3; then bulk_insert_edges alone on the RAW 16 x 2^22 tuples of RMAT-22, repeated pairs
          included, so multi-edge pairs occur — with the host phases (fh_last_bulk_phases_ns), the device phases of one
          fgpu_edges_build of the same tuples on the engine context (fgpu_prof_*), and on that graph the host leg's figures for
          one 1024-row 2-hop batch (operator22).  `load <scale>`: the twin comparison at that scale only.

  detach  the host layer's cascade delete: Graph::delete_nodes_bulk (one fgpu_nodes_detach per tensor, the label matrix and the
          adjacency) against the path that existed before it — one delete_edge per incident edge, then delete_node — on twin
          graphs of the distinct RMAT-12, RMAT-18 and RMAT-20 edges loaded with bulk_insert_edges, the same seeded 1 %, 10 % and
          100 % of the nodes, a host clock around delete + commit.  The bulk twin: one warm-up, median of 3, a fresh twin each.
          The edge-by-edge twin: one run under a deadline (60 s at RMAT-12, 10 s beyond), us per edge and the extrapolation
          when it did not finish.  Then the raw fgpu_nodes_detach on the RMAT-22 tensor of the load leg (UINT64 base + transposed
          pattern) for 1 % and 10 % of the nodes, with list and mt and on m alone, its device phases, beside one fgpu_mat_merge
          of the same matrix with 0.1 % deltas.  `detach <scale>`: the twin comparison at that scale only.

  edel    the host layer's explicit edge delete: Graph::delete_edges_bulk (one fgpu_edges_remove per tensor, one adjacency mask)
          against the path that existed before it — one delete_edge per edge — on twin graphs of the distinct RMAT-18 and
          RMAT-20 edges loaded with bulk_insert_edges, the same seeded, shuffled 10 % of the edges, a host clock around delete +
          commit.  The bulk twin: one warm-up, median of 3, a fresh twin each, with the host phases
          (fh_last_edge_delete_phases_ns).  The edge-by-edge twin: one run under a 10 s deadline, us per edge and the
          extrapolation.  Then the raw fgpu_edges_remove on the RMAT-22 tensor of the load leg (UINT64 base, transposed pattern,
          the multi-edge rows of the touched pairs) for a seeded 1 % and 10 % of the raw tuples, its device phases, beside one
          fgpu_mat_merge(m, NULL, dm) whose dm holds the same pairs.  `edel <scale>`: the twin comparison at that scale only.

  append  the host layer's bulk insert onto a loaded graph: Graph::append_edges_bulk (fgpu_edges_build + one fgpu_edges_union,
          every edge on the device) against what Graph::bulk_insert_edges does with the same batch — one pair that holds an
          edge sends it through set_all_from_slices whole — on twin graphs of the distinct RMAT-18 and RMAT-20 edges plus a
          second edge on a seeded 5 % of the pairs, loaded with bulk_insert_edges.  The batch is a seeded, shuffled 10 % as many
          new edges: half on loaded pairs (so a twentieth of those on multi-edge pairs), the rest on pairs the graph does not
          hold.  A host clock around the call + commit, one warm-up, median of 3, a fresh twin each, with the host phases
          (fh_last_append_phases_ns).  Then the raw fgpu_edges_union on the RMAT-22 tensor of the load leg for batches of 1 %
          and 10 % as many tuples built by fgpu_edges_build, its device phases, beside one fgpu_mat_merge(m, fwd, NULL) over
          the same pairs.  `append <scale>`: the twin comparison at that scale only.

  edges   the relationship-emitting CondTraverse batch: one 1024-row batch of (a:P)-[r]->(b) and one of (a:P)-[r]-(b) through
          Graph.cond_traverse_edges_batch (ONE fgpu_expand_edges) against cond_traverse_rows (the per-row path, 8 rows a call,
          stopped at a 10 s deadline and extrapolated) on one host-layer graph of the distinct RMAT-18 and RMAT-20 edges loaded
          with bulk_insert_edges, 1 % of the pairs multi-edge; medians of 5 calls after 2 warm-ups, with the stats of the call.
          Then the bare fgpu_expand_edges beside fgpu_expand_pairs32 on the same sources and the same tensor (fgpu_edges_build
          on the engine context), with its device phases.  `edges <scale>`: that scale only.

  varlen_batch   CondVarLenTraverse batches: (a:P)-[*1..2]->(b), (a:P)-[*1..3]->(b) and (a:P)-[*1..2]-(b) over 1024 :P rows of one
          RMAT-18 graph through Graph.var_len_traverse_batch (fgpu_expand_trails) against the loop of the per-row DFS over the same
          rows (stopped at a 10 s deadline and extrapolated), the rows compared inside the run; then the bare call with and
          without paths.  A pattern one device call cannot hold over all rows is timed on the lightest rows: the longest halved prefix,
          by out-degree, that fits.

  degrees  indegree() / outdegree() batches (fgpu_node_degrees) on the tensor fgpu_edges_build makes of the distinct RMAT-18, -20
          and -22 edges, 1 % of the pairs multi-edge: the 1024 first and all of the :P rows (a seeded sixteenth of the nodes), out
          and in, against fgpu_expand_edges with the other endpoint unbound + a bincount of its row column, in one process,
          medians of 5 after 2 warm-ups; at RMAT-18 also Graph.node_degrees against its per-row loop (stopped at a 10 s deadline
          and extrapolated).  Then the whole-graph form on the clean RMAT-22 tensor beside one fgpu_mat_row_degrees of m, and on
          the raw RMAT-22 stream with its multi-edge pairs.  `degrees <scale>`: the batches at that scale only.

usage: python tools/bench_paths.py [merge|expand|reach|host|load|detach|edel|append|edges|degrees|varlen_batch|pagerank|wcc|cdlp|harmonic|betweenness|sssp|sssp_sweep|hops|asp|all] [scale]
"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from falkordb_amd import engine


def timed(ctx, fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def deltas(ctx, A, frac, rng, valued=False):
    n, nnz = A.nrows, A.nvals
    k = max(1, int(nnz * frac))
    # tombstones: a uniformly random `frac` of the stored entries, drawn on the device (fgpu_mat_sample) — the first
    # version took them from rows [0, 65536] only, which clustered the touched rows and flattered the clean-word
    # merge path; pending adds: k uniformly random coordinates
    dm = A.sample(int(rng.integers(1, 1 << 30)), max(1, int(round(1.0 / frac))))
    pr = rng.integers(0, n, k, dtype=np.uint64)
    pc = rng.integers(0, n, k, dtype=np.uint64)
    dp = ctx.mat_from_coo(n, n, pr, pc, rng.integers(0, 1 << 40, k, dtype=np.uint64) if valued else None)
    return dp, dm


def bench_merge(ctx, scale):
    rng = np.random.default_rng(1)
    A = ctx.mat_rmat(scale)
    n, nnz = A.nrows, A.nvals
    dp, dm = deltas(ctx, A, 0.001, rng)
    for mode in (0, 2, 1):
        ctx.set_option("merge_mode", mode)
        dt, out = timed(ctx, lambda: A.merge(dp, dm))
        b_alg = 4 * (nnz + dp.nvals + dm.nvals) + 4 * out.nvals + 8 * (n + 1)
        print(json.dumps({"path": "delta_merge", "layers": "bool",
                          "kernel": ["entry-parallel", "row-wave", "entry-parallel, base marked per entry"][mode],
                          "scale": scale, "nnz_m": nnz, "nnz_dp": dp.nvals, "nnz_dm": dm.nvals,
                          "nnz_out": out.nvals, "ms": round(dt * 1e3, 3), "alg_bytes": b_alg,
                          "GBps": round(b_alg / dt / 1e9, 1), "frac_hbm": round(b_alg / dt / 8e12, 4)}), flush=True)
    ctx.set_option("merge_mode", 0)
    # UINT64 layers (Tensor::flush): values ride along, 8 B per entry each way
    rp, ci, _ = A.export_csr()
    r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
    V = ctx.mat_from_coo(n, n, r, ci, np.arange(len(ci), dtype=np.uint64))
    del r, ci, rp
    dpv, dmv = deltas(ctx, A, 0.001, rng, valued=True)
    dt, out = timed(ctx, lambda: V.merge(dpv, dmv), reps=3)
    b_alg = 12 * (nnz + dpv.nvals) + 4 * dmv.nvals + 12 * out.nvals + 8 * (n + 1)
    print(json.dumps({"path": "delta_merge", "layers": "u64", "kernel": "entry-parallel", "scale": scale,
                      "nnz_m": nnz, "nnz_out": out.nvals, "ms": round(dt * 1e3, 3), "alg_bytes": b_alg,
                      "GBps": round(b_alg / dt / 1e9, 1), "frac_hbm": round(b_alg / dt / 8e12, 4)}), flush=True)
    dt, out = timed(ctx, lambda: V.merge_pattern(dpv, dmv), reps=3)
    print(json.dumps({"path": "tensor_extract", "kernel": "entry-parallel", "scale": scale, "nnz_out": out.nvals,
                      "ms": round(dt * 1e3, 3)}), flush=True)
    dt, out = timed(ctx, lambda: A.transpose(), reps=3)
    print(json.dumps({"path": "transpose", "layers": "bool", "scale": scale, "ms": round(dt * 1e3, 3)}), flush=True)


def bench_expand(ctx, scale, hops=3, batch=1024, nbatches=3, rank=0, nranks=1, device="cpu"):
    """Under torch.distributed.run (WORLD_SIZE > 1) the batch is `batch` rows PER RANK, sharded by
    dist.expand_count_sharded over replicated layers (weak scaling, no data-path collective)."""
    from falkordb_amd import dist as fdist
    rng = np.random.default_rng(7)
    A = ctx.mat_rmat(scale)
    n, nnz = A.nrows, A.nvals
    dp, dm = deltas(ctx, A, 0.001, rng)
    for name, layers, cs in (("clean", ([A] * hops, None, None), True),
                             ("clean", ([A] * hops, None, None), False),
                             ("dirty-0.1%", ([A] * hops, [dp] * hops, [dm] * hops), True),
                             ("dirty-0.1%", ([A] * hops, [dp] * hops, [dm] * hops), False)):
        tot_t, tot_f, tot_n = 0.0, 0, 0
        for b in range(nbatches + 1):
            src = rng.choice(n, batch * nranks, replace=False).astype(np.uint64)
            ctx.sync()
            if nranks > 1:
                import torch.distributed as td
                td.barrier()
            t0 = time.perf_counter()
            out_nnz, flops = fdist.expand_count_sharded(
                lambda s_: engine.expand_count(ctx, s_, *layers, want_checksum=cs)[::2], src, rank, nranks, device)
            dt = time.perf_counter() - t0
            if b == 0:
                continue  # warm-up (transpose cache, pools)
            tot_t += dt; tot_f += flops; tot_n += out_nnz
        if rank:
            continue
        print(json.dumps({"path": "khop_expand", "layers": name, "result": "count + checksum" if cs else "count only",
                          "n_gpus": nranks, "scale": scale, "hops": hops, "batch_rows": batch * nranks,
                          "batches": nbatches, "ms_per_batch": round(tot_t / nbatches * 1e3, 3),
                          "flops_per_batch": tot_f // nbatches, "out_nnz_per_batch": tot_n // nbatches,
                          "GTEPS": round(tot_f / tot_t / 1e9, 2),
                          "alg_bytes_per_batch": int((4 * tot_f + 4 * tot_n) // nbatches),
                          "GBps": round((4 * tot_f + 4 * tot_n) / tot_t / 1e9, 1)}), flush=True)


def bench_reach(ctx, scale=19, edge_factor=38, hops=4, batch=1024):
    """BASELINE config 5 stand-in (LDBC SF100 is not available offline): ~0.5 M vertices / ~20 M edges,
    [*1..4] DISTINCT reachability of 1024 sources with dirty layers, the Delta fold on device, then the same
    query on the folded base."""
    rng = np.random.default_rng(5)
    A = ctx.mat_rmat(scale, edge_factor)
    n, nnz = A.nrows, A.nvals
    dp, dm = deltas(ctx, A, 0.001, rng)
    src = rng.choice(n, batch, replace=False).astype(np.uint64)
    for name, m, p_, d_ in (("dirty-0.1%", A, dp, dm), ("folded", None, None, None)):
        if m is None:
            dt_fold, m = timed(ctx, lambda: A.merge(dp, dm), reps=3)
            b_alg = 4 * (nnz + dp.nvals + dm.nvals) + 4 * m.nvals + 8 * (n + 1)
            print(json.dumps({"path": "delta_fold", "scale": scale, "nnz_m": nnz, "nnz_out": m.nvals,
                              "ms": round(dt_fold * 1e3, 3), "GBps": round(b_alg / dt_fold / 1e9, 1)}), flush=True)
        args = ([m] * hops, [p_] * hops if p_ else None, [d_] * hops if d_ else None)
        engine.expand_levels(ctx, src, *args)   # warm-up: transpose cache
        ctx.sync()
        t0 = time.perf_counter()
        r = engine.expand_levels(ctx, src, *args)
        dt = time.perf_counter() - t0
        print(json.dumps({"path": "varlen_reach", "layers": name, "scale": scale, "edges": m.nvals, "hops": hops,
                          "batch_rows": batch, "ms": round(dt * 1e3, 3), "hop_nnz": r["hop_nnz"],
                          "distinct_1_to_k": r["union_nnz"], "flops": r["flops"],
                          "GTEPS": round(r["flops"] / dt / 1e9, 2)}), flush=True)


def bench_pagerank(ctx, scale):
    """LAGr_PageRank's iteration on device: fixed 20 iterations (tol 0) so that the figure is per iteration;
    B_alg per iteration = 4 nnz (column ids of A') + 8 (N+1) (row pointers) + 6 x 4 N (t, d, w read / w, r written,
    sink bytes) with the gathers of w counted as cache traffic like the bitmap probes of the BFS formulas."""
    A = ctx.mat_rmat(scale)
    At = A.transpose()
    n, nnz = A.nrows, A.nvals
    engine.pagerank(ctx, A, At, None, 0.85, 0.0, 3)
    ctx.sync()
    its = 20
    t0 = time.perf_counter()
    scores, it = engine.pagerank(ctx, A, At, None, 0.85, 0.0, its)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    engine.pagerank(ctx, A, At, None, 0.85, 0.0, 3 * its)
    dt3 = time.perf_counter() - t0
    marginal = (dt3 - dt) / (2 * its)          # what one more iteration costs (the call's fixed part — set-up, the 4 N-byte copy-out — drops out)
    t1 = time.perf_counter()
    s2, it2 = engine.pagerank(ctx, A, At)
    dt2 = time.perf_counter() - t1
    b_alg = 4 * nnz + 8 * (n + 1) + 24 * n
    print(json.dumps({"path": "pagerank", "scale": scale, "vertices": n, "edges": nnz, "iterations": it,
                      "ms_per_iteration": round(dt / it * 1e3, 3), "ms_per_additional_iteration": round(marginal * 1e3, 3),
                      "alg_bytes_per_iteration": b_alg,
                      "GBps": round(b_alg * it / dt / 1e9, 1), "frac_hbm": round(b_alg * it / dt / 8e12, 4),
                      "default_run": {"tol": 1e-4, "iterations": it2, "ms": round(dt2 * 1e3, 3)},
                      "sum": round(float(scores.astype(np.float64).sum()), 6),
                      "note": "whole fgpu_pagerank call incl. one host sync per four iterations and the D2H of the scores"}), flush=True)


def load_edges(g, t, srcs, dsts, ids):
    """The host-layer load of a leg's graph: the bulk call from 2^18 edges on, edge by edge below."""
    if len(srcs) >= 1 << 18:
        g.bulk_insert_edges(t, srcs, dsts, ids)
    else:
        g.create_edges(t, srcs, dsts, ids)


def operator_figures(g, ctx, A, src):
    """One 1024-row 2-hop batch: CondTraverseOp::expand_batch (its own clock) against the bare fgpu_expand call."""
    from falkordb_amd import host
    spec = host.cond_spec(hops=[(["KNOWS"], []), (["KNOWS"], [])])
    srcl = src.tolist()
    for _ in range(2):
        (rows, _, _), nulls, flops = g.cond_traverse_batch(spec, srcl, as_arrays=True)
    t0 = time.perf_counter()
    (rows, _, _), nulls, flops = g.cond_traverse_batch(spec, srcl, as_arrays=True)
    t_host = time.perf_counter() - t0
    t_cpp = g.L.fh_last_op_ns() / 1e9
    for _ in range(2):
        rowptr, dest, fl = engine.expand(ctx, src, [A, A])
    t0 = time.perf_counter()
    rowptr, dest, fl = engine.expand(ctx, src, [A, A])
    t_raw = time.perf_counter() - t0
    assert len(rows) == len(dest) and fl == flops
    return {"hops": 2, "batch_rows": len(src), "rows_out": len(rows), "flops": flops, "ms_cpp_expand_batch": round(t_cpp * 1e3, 3),
            "ms_through_ctypes": round(t_host * 1e3, 3), "ms_bare_fgpu_expand": round(t_raw * 1e3, 3)}


def bench_load(scales=(18, 20), raw_scale=22):
    from falkordb_amd import host
    hc = host.Context(0)
    ctx = engine.Context(0)
    note = ("host clock around load + commit, both ending in a sync; twin graphs in one process, alternating, one warm-up, "
            "median of 3")
    for scale in scales:
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        ids = np.arange(len(ci), dtype=np.uint64)
        del rp
        A.free()

        def run(bulk):
            g = host.Graph(hc, n)
            t = g.add_type("KNOWS")
            t0 = time.perf_counter()
            st = g.bulk_insert_edges(t, r, ci, ids) if bulk else g.create_edges(t, r, ci, ids)
            t1 = time.perf_counter()
            g.commit()
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, (g.tensor_edge_count(t), g.tensor_state(t)["m"], len(g.layer(None, "dp"))), st

        times = {False: [], True: []}
        for rep in range(4):                     # (rep 0 warms both up)
            for bulk in (False, True):
                call, commit, state, st = run(bulk)
                assert state[0] == len(ci) and (not bulk or state == (len(ci), len(ci), 0)), state
                print(f"# load scale {scale} rep {rep} {'bulk' if bulk else 'create_edges'}: {call + commit:.3f} s", file=sys.stderr, flush=True)
                if rep:
                    times[bulk].append((call + commit, call, commit))
        med = {b: [float(np.median([x[k] for x in times[b]])) for k in range(3)] for b in times}
        print(json.dumps({"path": "graph_load", "scale": scale, "edges": len(ci),
                          "create_edges": {"s": round(med[False][0], 3), "call_s": round(med[False][1], 3), "commit_s": round(med[False][2], 3),
                                           "us_per_edge": round(med[False][0] / len(ci) * 1e6, 4)},
                          "bulk_insert_edges": {"s": round(med[True][0], 4), "call_s": round(med[True][1], 4), "commit_s": round(med[True][2], 4),
                                                "us_per_edge": round(med[True][0] / len(ci) * 1e6, 5), "stats": st},
                          "speedup": round(med[False][0] / med[True][0], 1), "note": note}), flush=True)
        del r, ci, ids
    if not raw_scale:
        return
    import oracle
    u, v = oracle.rmat_edges(raw_scale)          # the generator's stream before the duplicates collapse
    n = 1 << raw_scale
    ids = np.arange(len(u), dtype=np.uint64)
    runs = []
    for rep in range(4):
        g = host.Graph(hc, n)
        t = g.add_type("KNOWS")
        t0 = time.perf_counter()
        st = g.bulk_insert_edges(t, u, v, ids)
        dt = time.perf_counter() - t0
        runs.append((dt, g.last_bulk_phases_ms()))
        if rep == 0 and dt > 60:                 # (a load this slow is reported from its one run)
            break
    timed_runs = runs[1:] or runs
    k = int(np.argsort([x[0] for x in timed_runs])[len(timed_runs) // 2])
    dt, phases = timed_runs[k]
    assert g.tensor_edge_count(t) == len(u)
    ctx.prof_enable(True)
    pieces = engine.edges_build(ctx, n, n, u, v, ids, stats=True)
    ctx.sync()
    dev = {p["kernel"]: round(p["ms"], 3) for p in ctx.prof_read() if p["kernel"].startswith("eb_")}
    ctx.prof_enable(False)
    est = pieces[-1]
    del pieces
    print(json.dumps({"path": "graph_load_raw", "scale": raw_scale, "tuples": len(u), "distinct_pairs": st["distinct_pairs"],
                      "multi_pairs": st["multi_pairs"], "ids_in_multi_runs": est[2], "longest_run": est[3],
                      "unsorted_runs": st["unsorted_runs"], "bulk_insert_edges_s": round(dt, 3),
                      "us_per_edge": round(dt / len(u) * 1e6, 5), "runs_s": [round(x[0], 3) for x in runs],
                      "host_phases_ms": {k_: round(v_, 2) for k_, v_ in phases.items()},
                      "device_phases_ms": dev,
                      "note": "one warm-up, median of 3 (host clock, the call ends in a sync); host_phases = the C++ layer's own "
                              "clock: the fgpu_edges_build call (marshalling, H2D, sort, runs, transpose, read-back), fold + adopt, "
                              "me fill, adjacency union; device_phases = HIP events around the stages of one fgpu_edges_build of "
                              "the same tuples on the engine context (eb_h2d includes the staged host copies)"}), flush=True)
    A = ctx.mat_from_coo(n, n, u, v)
    src = np.random.default_rng(3).choice(n, 1024, replace=False).astype(np.uint64)
    print(json.dumps(dict({"path": "operator22", "scale": raw_scale}, **operator_figures(g, ctx, A, src))), flush=True)


def bench_detach(scales=(18, 20), small_scale=12, raw_scale=22, deadline_s=10.0):
    from falkordb_amd import host
    hc = host.Context(0)
    ctx = engine.Context(0)
    fracs = (0.01, 0.1, 1.0)

    def graph_of(scale):
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        A.free()
        return n, r, ci, np.arange(len(ci), dtype=np.uint64)

    def loaded(n, r, ci, ids):
        g = host.Graph(hc, n)
        t = g.add_type("KNOWS")
        g.bulk_insert_edges(t, r, ci, ids)
        g.commit()
        return g, t

    def nodes_of(n, frac):
        return np.sort(np.random.default_rng(int(frac * 1000)).choice(n, max(1, int(n * frac)), replace=False)).astype(np.uint64)

    def bulk(n, r, ci, ids, D, incident):
        ts = []
        for rep in range(4):                     # (rep 0 warms up; every rep deletes from a freshly loaded twin)
            g, t = loaded(n, r, ci, ids)
            t0 = time.perf_counter()
            rels, st = g.delete_nodes_bulk(D, stats=True, as_arrays=True)
            t1 = time.perf_counter()
            g.commit()
            t2 = time.perf_counter()
            assert st["edges_removed"] == incident == len(rels[0]) and g.tensor_edge_count(t) == len(ci) - incident
            ts.append((t2 - t0, t1 - t0, g.last_detach_phases_ms()))
            del rels, g
        k = int(np.argsort([x[0] for x in ts[1:]])[1]) + 1
        return ts[k]

    def edge_by_edge(n, r, ci, ids, D, mask, deadline):
        """today's path on a fresh twin: delete_edge per incident edge, then delete_node; stops at the deadline"""
        g, t = loaded(n, r, ci, ids)
        t0 = time.perf_counter()
        if len(ci) <= 1 << 20:                   # (the collection today's caller pays; past 2^20 edges the loaded arrays stand in)
            es = [e for e in g.tensor_iter_edges(t) if mask[e[0]] or mask[e[1]]]
        else:
            k = np.nonzero(mask[r] | mask[ci])[0]
            es = list(zip(r[k].tolist(), ci[k].tolist(), ids[k].tolist()))
        t_collect = time.perf_counter() - t0
        done = 0
        t0 = time.perf_counter()
        for s, d, i in es:
            g.delete_edge(t, s, d, i)
            done += 1
            if (done & 63) == 0 and time.perf_counter() - t0 > deadline:
                break
        finished = done == len(es)
        if finished:
            for v in D.tolist():
                g.delete_node(v)
            g.commit()
        dt = time.perf_counter() - t0
        return {"collect_s": round(t_collect, 3), "edges_done": done, "edges": len(es), "finished": finished, "s": round(dt, 3),
                "us_per_edge": round(dt / max(done, 1) * 1e6, 2),
                "s_extrapolated": round(dt / max(done, 1) * len(es), 2)}

    for scale in (small_scale,) + tuple(scales):
        n, r, ci, ids = graph_of(scale)
        for frac in fracs:
            D = nodes_of(n, frac)
            mask = np.zeros(n, dtype=bool)
            mask[D.astype(np.int64)] = True
            incident = int((mask[r] | mask[ci]).sum())
            total, call, phases = bulk(n, r, ci, ids, D, incident)
            ebe = edge_by_edge(n, r, ci, ids, D, mask, deadline_s * (6 if scale == small_scale else 1))
            ref = ebe["s"] if ebe["finished"] else ebe["s_extrapolated"]
            print(json.dumps({"path": "graph_detach", "scale": scale, "edges": len(ci), "nodes_deleted": len(D), "frac": frac,
                              "incident_edges": incident,
                              "delete_nodes_bulk": {"s": round(total, 5), "call_s": round(call, 5),
                                                    "us_per_edge": round(total / max(incident, 1) * 1e6, 5),
                                                    "host_phases_ms": {k_: round(v_, 3) for k_, v_ in phases.items()}},
                              "edge_by_edge": ebe, "quotient": round(ref / total, 1),
                              "note": "twin graphs loaded with bulk_insert_edges + commit in one process; host clock around delete + "
                                      "commit; bulk: one warm-up, median of 3, a fresh twin each; edge by edge: one run, stopped at "
                                      "its deadline (finished = false: s_extrapolated = us_per_edge x edges, and the quotient uses it)"}),
                  flush=True)
        del r, ci, ids
    if not raw_scale:
        return
    import oracle
    u, v = oracle.rmat_edges(raw_scale)
    n = 1 << raw_scale
    fwd, bwd, _, _, _ = engine.edges_build(ctx, n, n, u, v, np.arange(len(u), dtype=np.uint64))
    del u, v
    rng = np.random.default_rng(5)
    dp, dm = deltas(ctx, fwd, 0.001, rng, valued=True)
    t_merge, merged = timed(ctx, lambda: fwd.merge(dp, dm), reps=5, warm=2)
    del merged
    for frac in (0.01, 0.1):
        D = nodes_of(n, frac)
        t_call, res = timed(ctx, lambda: engine.nodes_detach(ctx, fwd, bwd, D, stats=True), reps=3, warm=1)
        st = res[-1]
        del res
        t_nolist, res = timed(ctx, lambda: engine.nodes_detach(ctx, fwd, None, D, want_list=False), reps=3, warm=1)
        del res
        ctx.prof_enable(True)
        res = engine.nodes_detach(ctx, fwd, bwd, D)
        ctx.sync()
        dev = {}
        for p in ctx.prof_read():
            if p["kernel"].startswith("dt_"):
                dev[p["kernel"]] = round(dev.get(p["kernel"], 0.0) + p["ms"], 3)
        ctx.prof_enable(False)
        del res
        print(json.dumps({"path": "nodes_detach_raw", "scale": raw_scale, "nnz": fwd.nvals, "frac": frac, "nodes": len(D), "stats": st[:6],
                          "ms_call_with_list_and_mt": round(t_call * 1e3, 3), "ms_call_m_only_no_list": round(t_nolist * 1e3, 3),
                          "device_phases_ms": dev, "ms_fgpu_mat_merge_0.1pct_deltas": round(t_merge * 1e3, 3),
                          "quotient_m_only_over_merge": round(t_nolist / t_merge, 2),
                          "note": "the UINT64 tensor base of the raw RMAT stream (fgpu_edges_build) and its transposed pattern; median "
                                  "of 3 synchronised calls after 1 warm-up, list read-back included; device_phases = HIP events of one "
                                  "more call (flags + scans of both passes, both emissions, the list's read-back); the merge is "
                                  "fgpu_mat_merge of the same matrix with 0.1 % valued adds and 0.1 % tombstones, median of 5"}),
              flush=True)


def bench_edel(scales=(18, 20), raw_scale=22, deadline_s=10.0):
    from falkordb_amd import host
    hc = host.Context(0)
    ctx = engine.Context(0)

    def loaded(n, r, ci, ids):
        g = host.Graph(hc, n)
        t = g.add_type("KNOWS")
        g.bulk_insert_edges(t, r, ci, ids)
        g.commit()
        return g, t

    for scale in scales:
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        ids = np.arange(len(ci), dtype=np.uint64)
        A.free()
        k = np.random.default_rng(100).choice(len(ci), len(ci) // 10, replace=False)    # a seeded tenth of the edges, shuffled
        tk = np.zeros(len(k), dtype=np.uint64)
        ts = []
        for rep in range(4):                     # (rep 0 warms up; every rep deletes from a freshly loaded twin)
            g, t = loaded(n, r, ci, ids)
            t0 = time.perf_counter()
            rels, st = g.delete_edges_bulk(tk, r[k], ci[k], ids[k], stats=True, as_arrays=True)
            t1 = time.perf_counter()
            g.commit()
            t2 = time.perf_counter()
            assert st["edges_removed"] == len(k) == len(rels[0]) and g.tensor_edge_count(t) == len(ci) - len(k)
            ts.append((t2 - t0, t1 - t0, g.last_edge_delete_phases_ms(), st))
            del rels, g
        total, call, phases, st = ts[int(np.argsort([x[0] for x in ts[1:]])[1]) + 1]
        g, t = loaded(n, r, ci, ids)             # the twin: one delete_edge per edge, stopped at the deadline
        es = list(zip(r[k].tolist(), ci[k].tolist(), ids[k].tolist()))
        done = 0
        t0 = time.perf_counter()
        for s, d, i in es:
            g.delete_edge(t, s, d, i)
            done += 1
            if (done & 63) == 0 and time.perf_counter() - t0 > deadline_s:
                break
        finished = done == len(es)
        if finished:
            g.commit()
        dt = time.perf_counter() - t0
        ref = dt if finished else dt / max(done, 1) * len(es)
        print(json.dumps({"path": "graph_edge_delete", "scale": scale, "edges": len(ci), "edges_deleted": len(k),
                          "delete_edges_bulk": {"s": round(total, 5), "call_s": round(call, 5),
                                                "us_per_edge": round(total / len(k) * 1e6, 5),
                                                "host_phases_ms": {k_: round(v_, 3) for k_, v_ in phases.items()},
                                                "stats": {k_: v_ for k_, v_ in st.items() if k_ != "per_type"}},
                          "edge_by_edge": {"edges_done": done, "finished": finished, "s": round(dt, 3),
                                           "us_per_edge": round(dt / max(done, 1) * 1e6, 2), "s_extrapolated": round(ref, 2)},
                          "quotient": round(ref / total, 1),
                          "note": "twin graphs loaded with bulk_insert_edges + commit in one process; host clock around delete + "
                                  "commit; bulk: one warm-up, median of 3, a fresh twin each; edge by edge: one run, stopped at "
                                  "its deadline (finished = false: s_extrapolated = us_per_edge x edges, and the quotient uses it)"}),
              flush=True)
        del r, ci, ids, g
    if not raw_scale:
        return
    import oracle
    u, v = (np.asarray(x, dtype=np.uint64) for x in oracle.rmat_edges(raw_scale))
    n = 1 << raw_scale
    ids = np.arange(len(u), dtype=np.uint64)
    fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, ids)
    mkey, moff, mids = np.array(mkey), np.array(moff), np.array(mids)
    for frac in (0.01, 0.1):
        k = np.random.default_rng(int(frac * 1000)).choice(len(u), int(len(u) * frac), replace=False)
        s, d, i = u[k], v[k], ids[k]
        t0 = time.perf_counter()
        keys = np.unique((s << np.uint64(32)) | d)                       # the multi-edge rows of the touched pairs, as the host layer gathers them
        at = np.searchsorted(mkey, keys)
        at = at[(at < len(mkey)) & (mkey[np.minimum(at, len(mkey) - 1)] == keys)]
        lens = (moff[at + 1] - moff[at]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        pos = np.repeat(moff[at].astype(np.int64) - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))
        rows = (mkey[at], off, mids[pos])
        t_gather = time.perf_counter() - t0
        t_call, res = timed(ctx, lambda: engine.edges_remove(ctx, fwd, bwd, s, d, i, *rows, stats=True), reps=3, warm=1)
        st = res[-1]
        del res
        ctx.prof_enable(True)
        res = engine.edges_remove(ctx, fwd, bwd, s, d, i, *rows)
        ctx.sync()
        dev = {}
        for p in ctx.prof_read():
            if p["kernel"].startswith(("er_", "dt_")):
                dev[p["kernel"]] = round(dev.get(p["kernel"], 0.0) + p["ms"], 3)
        ctx.prof_enable(False)
        del res
        dm = ctx.mat_from_coo(n, n, s, d)
        t_merge, merged = timed(ctx, lambda: fwd.merge(None, dm), reps=5, warm=2)
        nnz_merged = merged.nvals
        del merged
        print(json.dumps({"path": "edges_remove_raw", "scale": raw_scale, "nnz": fwd.nvals, "frac": frac, "triples": len(k),
                          "multi_rows_supplied": len(at), "ids_in_supplied_rows": int(off[-1]), "stats": st,
                          "ms_call": round(t_call * 1e3, 3), "ms_numpy_row_gather": round(t_gather * 1e3, 3),
                          "device_phases_ms": dev, "ms_call_outside_device_phases": round(t_call * 1e3 - sum(dev.values()), 3),
                          "ms_fgpu_mat_merge_m_minus_dm": round(t_merge * 1e3, 3),
                          "nnz_dm": dm.nvals, "nnz_merged": nnz_merged, "quotient_call_over_merge": round(t_call / t_merge, 2),
                          "note": "the UINT64 tensor base of the raw RMAT stream (fgpu_edges_build), its transposed pattern and the "
                                  "multi-edge rows of the touched pairs; median of 3 synchronised calls after 1 warm-up, host-side "
                                  "validation, H2D of triples and rows and the read-back of hit / taken / emptied included; "
                                  "device_phases = HIP events of one more call (er_h2d = the staged uploads, dt_emit = both emissions, er_readback = "
                                  "emptied pairs, taken and hit flags); outside them: validation and narrowing of the triples on the host, "
                                  "allocation, the row-pointer passes; the merge is "
                                  "fgpu_mat_merge(m, NULL, dm) with dm the BOOL matrix of the same pairs, median of 5 after 2 warm-up: "
                                  "it drops the whole pair where the call removes single edges"}), flush=True)
        del dm


def bench_edges(scales=(18, 20), deadline_s=10.0, k=1024):
    """The relationship-emitting CondTraverse batch (fgpu_expand_edges under Graph.cond_traverse_edges_batch) against the per-row
    path it takes over (cond_traverse_rows), and the bare call beside fgpu_expand_pairs32 on the same sources."""
    import ctypes as C
    from falkordb_amd import _ffi, host
    hc = host.Context(0)
    ctx = engine.Context(0)
    for scale in scales:
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        A.free()
        rng = np.random.default_rng(200 + scale)
        twice = rng.choice(len(ci), len(ci) // 100, replace=False)          # 1 % of the pairs hold a second edge
        u, v = np.concatenate([r, r[twice]]), np.concatenate([ci, ci[twice]])
        ids = np.arange(len(u), dtype=np.uint64)
        g = host.Graph(hc, n)
        t = g.add_type("KNOWS")
        g.bulk_insert_edges(t, u, v, ids)
        lid = g.add_label("P")
        srcs = rng.choice(n, k, replace=False)
        for x in np.concatenate([srcs, rng.choice(n, k, replace=False)]).tolist():
            g.label_node(int(x), lid)
        g.commit()
        srcs = srcs.tolist()
        none = [None] * k
        out = {"path": "cond_traverse_edges", "scale": scale, "edges": len(u), "multi_pairs": len(twice), "rows": k}
        for name, bidir in (("out", False), ("both", True)):
            spec = host.cond_spec(src_labels=["P"], hops=[(["KNOWS"], [])], emit=True, bidir=bidir)
            ts, res = [], None
            for rep in range(7):                                            # (2 warm-ups: the first builds the resident table)
                t0 = time.perf_counter()
                res = g.cond_traverse_edges_batch(spec, srcs, none, as_arrays=True)
                ts.append(time.perf_counter() - t0)
            cols, _, st = res
            done, got, t0 = 0, 0, time.perf_counter()
            while done < k:                                                 # the per-row path, 8 rows a call, up to the deadline
                got += len(g.cond_traverse_rows(spec, srcs[done:done + 8], none[:8]))
                done += 8
                if time.perf_counter() - t0 > deadline_s:
                    break
            dt = time.perf_counter() - t0
            ref = dt / done * k
            if done >= k:
                assert got == len(cols[0])
            out[name] = {"batch_ms_median_of_5": round(float(np.median(ts[2:])) * 1e3, 3), "batch_ms_all": [round(x * 1e3, 3) for x in ts],
                         "ids": int(len(cols[0])), "stats": st,
                         "per_row": {"rows_done": min(done, k), "finished": done >= k, "s": round(dt, 3),
                                     "ms_per_row": round(dt / done * 1e3, 3), "s_for_the_batch": round(ref, 3)},
                         "quotient": round(ref / float(np.median(ts[2:])), 1)}
        # the bare calls on the same sources: the tensor as fgpu_edges_build makes it, on the engine context
        fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, ids)
        multi = ctx.multi_new(np.array(mkey), np.array(moff), np.array(mids))
        for name, bidir in (("out", False), ("both", True)):
            t_call, res = timed(ctx, lambda: ctx.expand_edges(srcs, none, [fwd], None, None, [bwd], None, None, [multi],
                                                              bidirectional=bidir), reps=5, warm=2)
            out["raw_" + name] = {"ms": round(t_call * 1e3, 3), "stats": res[-1]}
            del res
        ctx.prof_enable(True)
        res = ctx.expand_edges(srcs, none, [fwd], None, None, [bwd], None, None, [multi])
        ctx.sync()
        out["raw_out"]["device_phases_ms"] = {p["kernel"]: round(p["ms"], 3) for p in ctx.prof_read() if p["kernel"].startswith("ee_")}
        ctx.prof_enable(False)
        del res
        src64 = np.asarray(srcs, dtype=np.uint64)
        arr = (C.c_void_p * 1)(fwd._h)

        def pairs32():
            prow, pdest = C.c_void_p(), _ffi.u32p()
            np_, fl = C.c_uint64(), C.c_uint64()
            _ffi.check(ctx.lib.fgpu_expand_pairs32(ctx._h, src64.ctypes.data_as(_ffi.u64p), k, arr, None, None, 1, None, None, 16,
                                                   C.byref(prow), C.byref(pdest), C.byref(np_), C.byref(fl)))
            ctx.lib.fgpu_free(ctx._h, prow)
            ctx.lib.fgpu_free(ctx._h, C.cast(pdest, C.c_void_p))
            return np_.value

        t_pairs, npairs = timed(ctx, pairs32, reps=5, warm=2)
        out["raw_pairs32"] = {"ms": round(t_pairs * 1e3, 3), "pairs": npairs}
        out["raw_quotient_edges_over_pairs32"] = round(out["raw_out"]["ms"] / (t_pairs * 1e3), 2)
        out["note"] = ("one host-layer graph loaded with bulk_insert_edges + commit (distinct RMAT edges, a second edge on a seeded 1 % of "
                       "the pairs), 1024 seeded sources carrying :P; host clock around the Python call, results copied out included; "
                       "batch: 2 warm-ups, median of 5; per row: cond_traverse_rows 8 rows a call up to the deadline (finished = "
                       "false: s_for_the_batch = ms_per_row x rows, and the quotient uses it); raw: the same tensor from "
                       "fgpu_edges_build on the engine context, median of 5 synchronised calls after 2 warm-ups, uploads and the "
                       "read-back of the columns included")
        print(json.dumps(out), flush=True)
        del g, fwd, bwd, multi


def bench_degrees(scales=(18, 20, 22), host_scale=18, whole_scale=22, deadline_s=10.0, k=1024):
    """indegree() / outdegree() batches (fgpu_node_degrees) against the only way the parent commit had to these numbers —
    fgpu_expand_edges with `to` unbound and a bincount of its row column — and, at host_scale, against the per-row host loop."""
    import ctypes as C
    import torch
    from falkordb_amd import _ffi, host
    ctx = engine.Context(0)
    for scale in scales:
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        A.free()
        rng = np.random.default_rng(300 + scale)
        twice = rng.choice(len(ci), len(ci) // 100, replace=False)          # 1 % of the pairs hold a second edge
        u, v = np.concatenate([r, r[twice]]), np.concatenate([ci, ci[twice]])
        ids = np.arange(len(u), dtype=np.uint64)
        P = np.sort(rng.choice(n, n // 16, replace=False)).astype(np.uint64)   # the :P rows: a seeded sixteenth of the nodes
        fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, ids)
        multi = ctx.multi_new(np.array(mkey), np.array(moff), np.array(mids))
        out = {"path": "node_degrees", "scale": scale, "edges": len(u), "multi_pairs": len(twice), "P_rows": len(P)}
        layers = [engine._hop_arrays(x) if x is not None else None for x in ([fwd], None, None, [bwd], None, None, [multi])]
        for name, nodes in (("first_1024", P[:k]), ("every_P_row", P)):
            unbound = np.full(len(nodes), (1 << 64) - 1, dtype=np.uint64)
            leg = {"rows": len(nodes)}
            for dname, kw in (("out", dict(out=True, incoming=False)), ("in", dict(out=False, incoming=True))):
                t_new, res = timed(ctx, lambda: ctx.node_degrees(nodes, [fwd], None, None, [bwd], None, None, [multi], **kw), reps=5, warm=2)
                deg = res[0] if dname == "out" else res[1]

                def old():   # (the arrays are made once, outside the clock: engine.expand_edges would encode two Python lists per call)
                    f, t = (nodes, unbound) if dname == "out" else (unbound, nodes)
                    prow, pfrom, pto, pid = _ffi.u32p(), _ffi.u32p(), _ffi.u32p(), _ffi.u64p()
                    cnt = C.c_uint64()
                    _ffi.check(ctx.lib.fgpu_expand_edges(ctx._h, engine._p(f), engine._p(t), len(nodes), *layers, 1, 0, None, None,
                                                         C.byref(prow), C.byref(pfrom), C.byref(pto), C.byref(pid), None, C.byref(cnt), None))
                    row, *_ = [ctx._take(p, cnt.value, dt) for p, dt in ((prow, np.uint32), (pfrom, np.uint32), (pto, np.uint32), (pid, np.uint64))]
                    return np.bincount(row, minlength=len(nodes))

                t_old, cnt = timed(ctx, old, reps=5, warm=2)
                assert np.array_equal(cnt.astype(np.uint64), deg)
                leg[dname] = {"node_degrees_ms": round(t_new * 1e3, 3), "expand_edges_bincount_ms": round(t_old * 1e3, 3),
                              "quotient": round(t_old / t_new, 2), "degree_sum": int(deg.sum()), "stats": res[2]}
            out[name] = leg
        ctx.prof_enable(True)
        ctx.node_degrees(P[:k], [fwd], None, None, [bwd], None, None, [multi])
        ctx.sync()
        out["first_1024"]["out"]["device_phases_ms"] = {p["kernel"]: round(p["ms"], 3) for p in ctx.prof_read() if p["kernel"].startswith("dg_")}
        ctx.prof_enable(False)
        del fwd, bwd, multi
        if scale == host_scale:   # the reference's per-row loop (DegreeFn::eval_row), 8 rows a call up to the deadline
            hc = host.Context(0)
            g = host.Graph(hc, n)
            t = g.add_type("KNOWS")
            g.bulk_insert_edges(t, u, v, ids)
            g.commit()
            ts = []
            for rep in range(7):
                t0 = time.perf_counter()
                got = g.node_degrees(P[:k])
                ts.append(time.perf_counter() - t0)
            done, t0 = 0, time.perf_counter()
            while done < k:
                per_row = g.node_degrees(P[done:done + 8], batched=False)
                assert np.array_equal(per_row, got[done:done + 8])
                done += 8
                if time.perf_counter() - t0 > deadline_s:
                    break
            dt = time.perf_counter() - t0
            out["host_first_1024_out"] = {"eval_batch_ms_median_of_5": round(float(np.median(ts[2:])) * 1e3, 3),
                                          "eval_row": {"rows_done": min(done, k), "finished": done >= k, "s": round(dt, 3),
                                                       "ms_per_row": round(dt / done * 1e3, 3), "s_for_the_batch": round(dt / done * k, 3)},
                                          "quotient": round(dt / done * k / float(np.median(ts[2:])), 1)}
            del g
            hc.close()
        out["note"] = ("the tensor fgpu_edges_build makes of the distinct RMAT edges plus a second edge on a seeded 1 % of the pairs, on the "
                       "engine context; :P = a seeded sixteenth of the node ids, ascending; both methods in this process on this tensor, "
                       "median of 5 synchronised calls after 2 warm-ups, uploads, read-backs and (for expand_edges) the bincount included; "
                       "host: Graph.node_degrees on a host-layer graph of the same edges, host clock around the Python call, eval_row 8 rows "
                       "a call up to the deadline (finished = false: s_for_the_batch = ms_per_row x rows)")
        print(json.dumps(out), flush=True)
    if not whole_scale:
        ctx.close()
        return
    # the whole-graph form: the clean tensor beside one fgpu_mat_row_degrees of m, then the raw stream with its multi-edge pairs
    import oracle
    n = 1 << whole_scale
    A = ctx.mat_rmat(whole_scale)
    rp, ci, _ = A.export_csr()
    r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
    ci = np.array(ci, dtype=np.uint64)
    fwd, bwd, *_ = engine.edges_build(ctx, n, n, r, ci, np.arange(len(ci), dtype=np.uint64))
    dev = torch.empty(n, dtype=torch.int32, device="cuda")

    def row_degrees():
        fwd.row_degrees(dev.data_ptr())
        ctx.sync()
        return dev.cpu().numpy()

    t_rd, rd = timed(ctx, row_degrees, reps=5, warm=2)
    t_out, res = timed(ctx, lambda: ctx.node_degrees(None, [fwd]), reps=5, warm=2)
    assert np.array_equal(res[0], rd.astype(np.uint64))
    t_both, both = timed(ctx, lambda: ctx.node_degrees(None, [fwd], mt_m=[bwd], incoming=True), reps=5, warm=2)
    line = {"path": "node_degrees_whole_graph", "scale": whole_scale, "n": n,
            "clean": {"edges": len(ci), "out_ms": round(t_out * 1e3, 3), "out_and_in_ms": round(t_both * 1e3, 3),
                      "mat_row_degrees_plus_copy_ms": round(t_rd * 1e3, 3), "stats_out": res[2], "stats_both": both[2]}}
    del fwd, bwd, res, both
    A.free()
    u, v = (np.asarray(x, dtype=np.uint64) for x in oracle.rmat_edges(whole_scale))
    fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, np.arange(len(u), dtype=np.uint64))
    multi = ctx.multi_new(np.array(mkey), np.array(moff), np.array(mids))
    t_out, res = timed(ctx, lambda: ctx.node_degrees(None, [fwd], multi=[multi]), reps=5, warm=2)
    t_both, both = timed(ctx, lambda: ctx.node_degrees(None, [fwd], mt_m=[bwd], multi=[multi], incoming=True), reps=5, warm=2)
    assert int(res[0].sum()) == len(u) == int(both[1].sum())
    ctx.prof_enable(True)
    ctx.node_degrees(None, [fwd], mt_m=[bwd], multi=[multi], incoming=True)
    ctx.sync()
    phases = {p["kernel"]: round(p["ms"], 3) for p in ctx.prof_read() if p["kernel"].startswith("dg_")}
    ctx.prof_enable(False)
    line["raw_stream"] = {"tuples": len(u), "pairs": fwd.nvals, "multi_pairs": multi.size()[0], "out_ms": round(t_out * 1e3, 3),
                          "out_and_in_ms": round(t_both * 1e3, 3), "stats_out": res[2], "stats_both": both[2],
                          "device_phases_ms_both": phases}
    line["note"] = ("median of 5 synchronised calls after 2 warm-ups, the k-word results copied to pageable host arrays included; clean: "
                    "the distinct edges, no table given, so every triple is the row-pointer tier's; fgpu_mat_row_degrees writes 32-bit "
                    "counts to device memory, timed with a device-to-host copy of them; raw_stream: every generated tuple, repeated "
                    "pairs as multi-edges with their table, so every entry goes through the entry tier")
    print(json.dumps(line), flush=True)
    ctx.close()


def bench_varlen(scale=18, deadline_s=10.0, k=1024, fit_items=1 << 26):
    """CondVarLenTraverse batches (fgpu_expand_trails under Graph.var_len_traverse_batch) against the loop of expand_row over the
    same rows (fh_var_len_traverse row by row: the path every batch took before), and the bare call with and without paths."""
    import ctypes as C
    from falkordb_amd import _ffi, host
    hc = host.Context(0)
    ctx = engine.Context(0)
    A = ctx.mat_rmat(scale)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
    ci = np.array(ci, dtype=np.uint64)
    A.free()
    deg = np.diff(rp).astype(np.int64)
    rng = np.random.default_rng(300 + scale)
    twice = rng.choice(len(ci), len(ci) // 100, replace=False)              # 1 % of the pairs hold a second edge
    u, v = np.concatenate([r, r[twice]]), np.concatenate([ci, ci[twice]])
    ids = np.arange(len(u), dtype=np.uint64)
    g = host.Graph(hc, n)
    t = g.add_type("KNOWS")
    g.bulk_insert_edges(t, u, v, ids)
    lid = g.add_label("P")
    srcs = rng.choice(n, k, replace=False)
    for x in srcs.tolist():
        g.label_node(int(x), lid)
    g.commit()
    fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, ids)
    multi = ctx.multi_new(np.array(mkey), np.array(moff), np.array(mids))
    quart = lambda ts: [round(float(x) * 1e3, 3) for x in np.percentile(ts, [25, 50, 75])]

    def one_row(start, lo, hi, bidir):                                      # fh_var_len_traverse without the Python row tuples
        of, ot, op_, off = host.u64p(), host.u64p(), host.u64p(), host.u64p()
        cnt = C.c_uint64()
        host._ck(g.L.fh_var_len_traverse(g.h, b"KNOWS", b"", 0, 1 if bidir else 0, C.c_uint32(lo), C.c_uint32(hi), C.c_uint64(start),
                                         C.c_int64(-1), 0, 1, C.byref(of), C.byref(ot), C.byref(op_), C.byref(off), C.byref(cnt), None))
        ft = (host._take(of, cnt.value), host._take(ot, cnt.value))
        for q in (op_, off):
            g.L.fh_free(C.cast(q, C.c_void_p))
        return ft

    for name, lo, hi, bidir in (("out_1_2", 1, 2, False), ("out_1_3", 1, 3, False), ("both_1_2", 1, 2, True)):
        out = {"path": "varlen_batch", "pattern": name, "scale": scale, "edges": len(u), "multi_pairs": len(twice)}
        # the rows: all k when one device call holds them in fit_items; else the k rows lightest first (by out-degree) and the
        # longest halved prefix of those that fits
        rows, st, order = k, [], srcs
        while rows:
            try:
                res = ctx.expand_trails(order[:rows], None, [fwd], None, None, [bwd], None, None, [multi], bidirectional=bidir,
                                        min_hops=lo, max_hops=hi, max_items=fit_items, stats_out=st)
                del res
                break
            except engine.FgpuError as e:
                if e.code != _ffi.FGPU_INSUFFICIENT_SPACE:
                    raise
                out.setdefault("all_rows_hold_more_than", int(st[7]))
                order = srcs[np.argsort(deg[srcs], kind="stable")]
                rows //= 2
        if rows == 0:
            out.update(rows=0, rows_asked=k, stats=st, note="not even the lightest row fits one device call of fit_items")
            print(json.dumps(out), flush=True)
            continue
        budget = max(1 << 22, 1 << int(st[7]).bit_length())
        out.update(rows=rows, rows_asked=k, device_budget=budget, stats=st)
        sub = order[:rows]
        for paths in (False, True):                                         # the bare call
            ts = []
            for rep in range(7):
                t0 = time.perf_counter()
                res = ctx.expand_trails(sub, None, [fwd], None, None, [bwd], None, None, [multi], bidirectional=bidir, paths=paths,
                                        min_hops=lo, max_hops=hi, max_items=budget)
                ctx.sync()
                ts.append(time.perf_counter() - t0)
                del res
            out["raw_paths" if paths else "raw"] = {"ms_q1_median_q3_of_5": quart(ts[2:])}
        ts, cols = [], None
        for rep in range(7):                                                # the operator's batch (2 warm-ups)
            t0 = time.perf_counter()
            cols, hst = g.var_len_traverse_batch(sub, types=["KNOWS"], min_hops=lo, max_hops=hi, bidirectional=bidir,
                                                 device_budget=budget, as_arrays=True)
            ts.append(time.perf_counter() - t0)
        # the loop of expand_row, lightest rows first (a row cannot be interrupted: one is started only while the rows done so
        # far predict that it ends by the deadline), each row compared with its part of the batch
        per = np.bincount(cols[0].astype(np.int64), minlength=rows)
        first = np.concatenate([[0], np.cumsum(per)])
        light = np.argsort(per, kind="stable")
        one_row(int(sub[light[0]]), lo, hi, bidir)                          # (warm)
        done, at, equal, rate, t0 = 0, 0, True, 2e-4, time.perf_counter()   # (rate: s per emitted row, until one is measured)
        for i in light.tolist():
            if done and (time.perf_counter() - t0) + per[i] * rate > deadline_s:
                break
            if not done and per[i] * rate > 10 * deadline_s:
                break
            f, to = one_row(int(sub[i]), lo, hi, bidir)
            equal = equal and np.array_equal(f, cols[1][first[i]:first[i + 1]]) and np.array_equal(to, cols[2][first[i]:first[i + 1]])
            at += len(f)
            done += 1
            if at >= 1000:                                                  # (a handful of rows says nothing about a hub)
                rate = (time.perf_counter() - t0) / at
            print("loop", name, done, at, round(time.perf_counter() - t0, 2), file=sys.stderr, flush=True)
        dt = time.perf_counter() - t0
        assert equal, "the batch and the loop differ"
        ref = dt / at * len(cols[0]) if at else float("nan")              # (by emitted rows: the hubs carry the time)
        out["batch"] = {"ms_q1_median_q3_of_5": quart(ts[2:]), "emissions": int(len(cols[0])), "stats": hst}
        out["loop"] = {"rows_done": done, "finished": done >= rows, "emissions_done": at, "s": round(dt, 3),
                       "s_for_the_batch": round(ref, 3), "rows_equal_to_the_batch": bool(equal)}
        out["quotient_loop_over_batch"] = round(ref / float(np.median(ts[2:])), 1)
        out["note"] = ("one host-layer graph of the distinct RMAT edges loaded with bulk_insert_edges + commit (a second edge on a "
                       "seeded 1 % of the pairs), the seeded :P sources as rows; host clock around the call, the columns copied out "
                       "as arrays included on both sides; batch: 2 warm-ups, quartiles of 5; loop: fh_var_len_traverse row by row "
                       "(the unchanged expand_row), lightest rows first, none started past the deadline, then extrapolated by emitted "
                       "rows, every row's (from, to) compared with the batch's inside the run; rows < rows_asked: one device call "
                       "did not hold the pattern over all rows in fit_items (all_rows_hold_more_than: the items counted when it "
                       "gave up), so the rows were ordered by out-degree and the longest halved prefix that fits was timed; raw: the same "
                       "tensor from fgpu_edges_build on the engine context, synchronised calls, uploads and read-back included")
        print(json.dumps(out), flush=True)


def bench_append(scales=(18, 20), raw_scale=22):
    from falkordb_amd import host
    hc = host.Context(0)
    ctx = engine.Context(0)
    for scale in scales:
        A = ctx.mat_rmat(scale)
        n = A.nrows
        rp, ci, _ = A.export_csr()
        r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
        ci = np.array(ci, dtype=np.uint64)
        A.free()
        E = len(ci)
        rng = np.random.default_rng(200 + scale)
        dup = rng.choice(E, E // 20, replace=False)                     # a second edge on 5 % of the pairs
        ls, ld = np.r_[r, r[dup]], np.r_[ci, ci[dup]]
        lid = np.arange(len(ls), dtype=np.uint64)
        nb = E // 10
        on = rng.choice(E, nb // 2, replace=False)                       # half of the batch lands on loaded pairs
        keys = (r << np.uint64(32)) | ci                                 # (ascending: CSR order)
        fs, fd = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        while len(fs) < nb - nb // 2:                                    # ... the rest on pairs the graph does not hold
            s, d = rng.integers(0, n, nb, dtype=np.uint64), rng.integers(0, n, nb, dtype=np.uint64)
            k = (s << np.uint64(32)) | d
            at = np.minimum(np.searchsorted(keys, k), E - 1)
            new = keys[at] != k
            fs, fd = np.r_[fs, s[new]], np.r_[fd, d[new]]
        mix = rng.permutation(nb)
        bs, bd = np.r_[r[on], fs[:nb - nb // 2]][mix], np.r_[ci[on], fd[:nb - nb // 2]][mix]
        bi = np.arange(len(ls), len(ls) + nb, dtype=np.uint64)
        on_multi = int(np.isin(on, dup).sum())

        def loaded():
            g = host.Graph(hc, n)
            t = g.add_type("KNOWS")
            g.bulk_insert_edges(t, ls, ld, lid)
            g.commit()
            return g, t

        ts = []
        for rep in range(4):                     # (rep 0 warms up; every rep appends to freshly loaded twins)
            g, t = loaded()
            t0 = time.perf_counter()
            st = g.append_edges_bulk(t, bs, bd, bi)
            t1 = time.perf_counter()
            g.commit()
            t2 = time.perf_counter()
            phases = g.last_append_phases_ms()
            g2, _ = loaded()
            t3 = time.perf_counter()
            st2 = g2.bulk_insert_edges(t, bs, bd, bi)
            t4 = time.perf_counter()
            g2.commit()
            t5 = time.perf_counter()
            assert st2["fallback_edges"] == nb and st["edges"] == nb
            assert g.tensor_edge_count(t) == g2.tensor_edge_count(t) == len(ls) + nb
            assert g.tensor_state(t)["multi_pairs"] == g2.tensor_state(t)["multi_pairs"]
            ts.append((t2 - t0, t1 - t0, phases, st, t5 - t3, t4 - t3))
            del g, g2
        total, call, phases, st, _, _ = ts[int(np.argsort([x[0] for x in ts[1:]])[1]) + 1]
        _, _, _, _, ftotal, fcall = ts[int(np.argsort([x[4] for x in ts[1:]])[1]) + 1]
        print(json.dumps({"path": "graph_append", "scale": scale, "edges_loaded": len(ls), "pairs_loaded": E,
                          "multi_pairs_loaded": len(dup), "edges_appended": nb, "on_loaded_pairs": nb // 2,
                          "on_multi_pairs": on_multi,
                          "append_edges_bulk": {"s": round(total, 5), "call_s": round(call, 5), "us_per_edge": round(total / nb * 1e6, 5),
                                                "host_phases_ms": {k_: round(v_, 3) for k_, v_ in phases.items()}, "stats": st},
                          "bulk_insert_edges_fallback": {"s": round(ftotal, 5), "call_s": round(fcall, 5),
                                                         "us_per_edge": round(ftotal / nb * 1e6, 5)},
                          "quotient": round(ftotal / total, 1),
                          "note": "twin graphs loaded with bulk_insert_edges + commit in one process; host clock around the call + "
                                  "commit; one warm-up, median of 3, fresh twins each; the twin's bulk_insert_edges takes "
                                  "set_all_from_slices for the whole batch (fallback_edges = the batch), which is what this batch cost "
                                  "before append_edges_bulk"}), flush=True)
        del r, ci, ls, ld, lid, keys
    if not raw_scale:
        return
    import oracle
    u, v = (np.asarray(x, dtype=np.uint64) for x in oracle.rmat_edges(raw_scale))
    n = 1 << raw_scale
    fwd, bwd, mkey, moff, mids = engine.edges_build(ctx, n, n, u, v, np.arange(len(u), dtype=np.uint64))
    mkey, moff, mids = np.array(mkey), np.array(moff), np.array(mids)
    for frac in (0.01, 0.1):
        rng = np.random.default_rng(int(frac * 1000))
        nb = int(len(u) * frac)
        k = rng.choice(len(u), nb // 2, replace=False)
        s = np.r_[u[k], rng.integers(0, n, nb - nb // 2, dtype=np.uint64)]
        d = np.r_[v[k], rng.integers(0, n, nb - nb // 2, dtype=np.uint64)]
        mix = rng.permutation(nb)
        s, d = s[mix], d[mix]
        t0 = time.perf_counter()
        bf, bb, bk, bo, bids = engine.edges_build(ctx, n, n, s, d, np.arange(len(u), len(u) + nb, dtype=np.uint64))
        ctx.sync()
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        keys = np.unique((s << np.uint64(32)) | d)                       # the multi-edge rows of the touched pairs, as the host layer gathers them
        at = np.searchsorted(mkey, keys)
        at = at[(at < len(mkey)) & (mkey[np.minimum(at, len(mkey) - 1)] == keys)]
        lens = (moff[at + 1] - moff[at]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        pos = np.repeat(moff[at].astype(np.int64) - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))
        rows = (mkey[at], off, mids[pos])
        t_gather = time.perf_counter() - t0
        t_call, res = timed(ctx, lambda: engine.edges_union(ctx, fwd, bwd, *rows, bf, bb, bk, bo, bids, stats=True), reps=3, warm=1)
        st = res[-1]
        del res
        ctx.prof_enable(True)
        res = engine.edges_union(ctx, fwd, bwd, *rows, bf, bb, bk, bo, bids)
        ctx.sync()
        dev = {}
        for p in ctx.prof_read():
            if p["kernel"].startswith("eu_"):
                dev[p["kernel"]] = round(dev.get(p["kernel"], 0.0) + p["ms"], 3)
        ctx.prof_enable(False)
        del res
        t_merge, merged = timed(ctx, lambda: fwd.merge(bf, None), reps=5, warm=2)
        nnz_merged = merged.nvals
        del merged
        print(json.dumps({"path": "edges_union_raw", "scale": raw_scale, "nnz": fwd.nvals, "frac": frac, "tuples": nb,
                          "nnz_fwd": bf.nvals, "a_rows_supplied": len(at), "ids_in_a_rows": int(off[-1]), "b_rows": len(bk), "stats": st,
                          "ms_call": round(t_call * 1e3, 3), "ms_edges_build_of_the_batch": round(t_build * 1e3, 3),
                          "ms_numpy_row_gather": round(t_gather * 1e3, 3), "device_phases_ms": dev,
                          "ms_call_outside_device_phases": round(t_call * 1e3 - sum(dev.values()), 3),
                          "ms_fgpu_mat_merge_m_with_fwd": round(t_merge * 1e3, 3), "nnz_merged": nnz_merged,
                          "quotient_call_over_merge": round(t_call / t_merge, 2),
                          "note": "the UINT64 tensor base of the raw RMAT stream (fgpu_edges_build), its transposed pattern, a built "
                                  "batch and the multi-edge rows of the touched pairs; median of 3 synchronised calls after 1 warm-up, "
                                  "host-side validation, H2D of the rows and the read-back of the out rows included; device_phases = "
                                  "HIP events of one more call (eu_h2d = the staged uploads, eu_place = both placements, eu_readback = "
                                  "the out rows); outside them: validation of the rows on the host, allocation, the histogram, its "
                                  "scan and the row-pointer passes; the merge is fgpu_mat_merge(m, fwd, NULL) on the forward matrix "
                                  "alone, median of 5 after 2 warm-up: the batch's value wins, no promotion, no ids, no mt"}), flush=True)
        del bf, bb


def bench_host(scale):
    """expand_batch through libfalkor_host.so (label probes, layer waits, result hand-off) vs bare fgpu_expand."""
    from falkordb_amd import host
    hc = host.Context(0)
    ctx = engine.Context(0)
    A = ctx.mat_rmat(scale)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp).astype(np.int64))
    g = host.Graph(hc, n)
    t = g.add_type("KNOWS")
    lp = g.add_label("P")
    t0 = time.perf_counter()
    load_edges(g, t, r, ci, np.arange(len(ci), dtype=np.uint64))
    g.commit()
    build = time.perf_counter() - t0
    rng = np.random.default_rng(3)
    src = rng.choice(n, 1024, replace=False).astype(np.uint64)
    spec = host.cond_spec(hops=[(["KNOWS"], []), (["KNOWS"], [])])
    srcl = src.tolist()
    for _ in range(2):
        (rows, _, _), nulls, flops = g.cond_traverse_batch(spec, srcl, as_arrays=True)
    t0 = time.perf_counter()
    (rows, _, _), nulls, flops = g.cond_traverse_batch(spec, srcl, as_arrays=True)
    t_host = time.perf_counter() - t0
    import ctypes
    g.L.fh_last_op_ns.restype = ctypes.c_uint64
    t_cpp = g.L.fh_last_op_ns() / 1e9
    for _ in range(2):
        rowptr, dest, fl = engine.expand(ctx, src, [A, A])
    t0 = time.perf_counter()
    rowptr, dest, fl = engine.expand(ctx, src, [A, A])
    t_raw = time.perf_counter() - t0
    assert len(rows) == len(dest) and fl == flops
    print(json.dumps({"path": "host_expand_batch", "scale": scale, "hops": 2, "batch_rows": 1024, "rows_out": len(rows),
                      "flops": flops, "ms_cpp_expand_batch": round(t_cpp * 1e3, 3), "ms_through_ctypes": round(t_host * 1e3, 3), "ms_bare_fgpu_expand": round(t_raw * 1e3, 3),
                      "graph_load_s": round(build, 2),
                      "note": "cpp = CondTraverseOp::expand_batch alone (label probes, fgpu_expand, result columns); through_ctypes adds the test harness' copies into numpy"}), flush=True)


def bench_wcc(ctx, scale):
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    At = A.transpose()
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    S = ctx.mat_from_coo(n, n, np.concatenate([rows, ci]), np.concatenate([ci, rows]))   # A (+) A'
    del rp, ci, rows
    for label, a, at in (("A+At", A, At), ("symmetric", S, None)):
        nnz = a.nvals
        bound_ms = (4 * nnz + 4 * (n + 1)) / 8e12 * 1e3
        out = ctx.host_array(n, np.int64)
        for mode in (1, 2):
            ctx.set_option("wcc_mode", mode)
            t, (_, st) = timed(ctx, lambda: engine.wcc(ctx, a, at, stats=True, out=out), reps=10, warm=2)
            print(json.dumps({"path": "wcc", "scale": scale, "input": label, "wcc_mode": mode, "n": n, "nnz": nnz,
                              "ms": round(t * 1e3, 3), "components": st[0], "entries_read": st[1], "link_launches": st[2],
                              "giant": st[3], "full_pass_bound_ms": round(bound_ms, 4),
                              "note": "host clock around a synchronised call, median of 10 after 2 warm-up; bound = "
                                      "(4 nnz(A) + 4 (n + 1)) bytes at 8 TB/s, one read of the CSR"}), flush=True)
    ctx.set_option("wcc_mode", 0)


def bench_cdlp(ctx, scale):
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    S = ctx.mat_from_coo(n, n, np.concatenate([rows, ci]), np.concatenate([ci, rows]))   # A (+) A'
    del rp, ci, rows, A
    nnz = S.nvals
    out = ctx.host_array(n, np.int64)
    t, (_, st) = timed(ctx, lambda: engine.cdlp(ctx, S, None, 10, stats=True, out=out), reps=10, warm=2)
    its = max(st[0], 1)
    # the marginal iteration: a 1-iteration call carries the whole fixed part (row classes, hub scratch, the 8 n-byte copy-out)
    t1, _ = timed(ctx, lambda: engine.cdlp(ctx, S, None, 1, out=out), reps=10, warm=1)
    per_iter = (t - t1) / (its - 1) if its > 1 else t
    # fgpu_pagerank on the same matrix (S is its own transpose), tol 0: fixed iteration counts, the marginal iteration
    pr = {}
    for k in (10, 30):
        pr[k], _ = timed(ctx, lambda: engine.pagerank(ctx, S, S, None, 0.85, 0.0, k), reps=5, warm=1)
    pr_iter = (pr[30] - pr[10]) / 20
    b_iter = 4 * nnz + 4 * nnz + 8 * n
    print(json.dumps({"path": "cdlp", "scale": scale, "n": n, "nnz": nnz, "itermax": 10, "ms": round(t * 1e3, 3),
                      "iterations": st[0], "changed_last": st[1], "entries_read": st[2], "distinct_labels": st[3],
                      "ms_one_iteration_call": round(t1 * 1e3, 3), "ms_per_iteration": round(per_iter * 1e3, 3),
                      "ms_per_iteration_whole_call": round(t / its * 1e3, 3),
                      "bytes_per_iteration": b_iter, "share_of_8TBps": round(b_iter / 8e12 / per_iter, 4) if per_iter > 0 else None,
                      "pagerank_ms_per_iteration": round(pr_iter * 1e3, 3),
                      "ratio_to_pagerank": round(per_iter / pr_iter, 2) if pr_iter > 0 else None,
                      "note": "host clock around a synchronised call, median of 10 after 2 warm-up; ms_per_iteration = (the "
                              "10-iteration call - a 1-iteration call) / (iterations - 1); bytes = 4 nnz + 4 nnz + 8 n; pagerank = "
                              "fgpu_pagerank on the same matrix, (30 iterations - 10 iterations) / 20"}), flush=True)


def bench_harmonic(ctx, scale):
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    n, nnz = A.nrows, A.nvals
    out = (ctx.host_array(n, np.float64), ctx.host_array(n, np.int64))
    t, (_, _, _, st) = timed(ctx, lambda: engine.harmonic(ctx, A, stats=True, out=out), reps=5, warm=1)
    entries, gathered = ctx.get_option("harmonic_last_entries"), ctx.get_option("harmonic_last_gathered")
    E = ctx.mat_new(n, n)
    t0, _ = timed(ctx, lambda: engine.harmonic(ctx, E, out=out), reps=5, warm=1)
    its = st[0] + 1                                           # the iteration that changed nothing ran as well
    work = max(t - t0, 1e-9)
    print(json.dumps({"path": "harmonic", "scale": scale, "n": n, "nnz": nnz, "ms": round(t * 1e3, 3),
                      "ms_fixed_part": round(t0 * 1e3, 3), "iterations_changing": st[0], "iterations_run": its,
                      "sketch_changes": st[1], "largest_reachable": st[2], "nonzero_scores": st[3],
                      "ms_per_iteration": round(work / its * 1e3, 3), "ms_per_iteration_whole_call": round(t / its * 1e3, 3),
                      "entries_of_recomputed_rows": entries, "sketches_gathered": gathered,
                      "TBps_entries_of_recomputed_rows": round(entries * 1024 / work / 1e12, 3),
                      "TBps_sketches_gathered": round(gathered * 1024 / work / 1e12, 3),
                      "share_of_5.5TBps_entries": round(entries * 1024 / work / 5.5e12, 3),
                      "share_of_5.5TBps_gathered": round(gathered * 1024 / work / 5.5e12, 3),
                      "note": "host clock around a synchronised call, median of 5 after 1 warm-up; fixed part = the same call on an "
                              "empty n x n matrix; per-iteration and TB/s figures use the call less the fixed part"}), flush=True)


def bench_msf(ctx, scale):
    """fgpu_msf on the symmetrised R-MAT graph: every pair's weight is a fixed hash of (lo, hi) mapped into [0, 100); a second run
    on the BOOL pattern (all ties: the pair order alone decides).  The yardstick beside it is fgpu_wcc with wcc_mode 2 on the same
    matrix: one link pass over every entry."""
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    n = A.nrows
    rp, ci, _ = A.export_csr()
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    keep = rows != ci
    lo, hi = np.minimum(rows, ci)[keep], np.maximum(rows, ci)[keep]
    key = np.unique(lo * np.uint64(n) + hi)                  # every unordered pair once
    lo, hi = key // np.uint64(n), key % np.uint64(n)
    del rp, ci, rows, keep, A
    h = key * np.uint64(0x9E3779B97F4A7C15)                  # (mod 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    w = (h >> np.uint64(11)).astype(np.float64) * (100.0 / 2.0**53)
    r2, c2 = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    W = ctx.mat_from_coo(n, n, r2, c2, np.concatenate([w, w]).view(np.uint64))
    S = ctx.mat_from_coo(n, n, r2, c2)
    del lo, hi, key, h, w, r2, c2
    nnz = W.nvals
    out = ctx.host_array(n, np.int64)
    ctx.set_option("wcc_mode", 2)
    t_wcc, (_, wst) = timed(ctx, lambda: engine.wcc(ctx, S, None, stats=True, out=out), reps=5, warm=2)
    ctx.set_option("wcc_mode", 0)
    for label, m, per_entry in (("weighted", W, 12), ("bool", S, 4)):
        t, res = timed(ctx, lambda: engine.msf(ctx, m, stats=True, out=out), reps=5, warm=2)
        st = res[4]
        per_round = [ctx.get_option("msf_last_entries_round%d" % k) for k in range(min(st[0] + 1, 32))]
        print(json.dumps({"path": "msf", "scale": scale, "input": label, "n": n, "nnz": nnz, "ms": round(t * 1e3, 3),
                          "rounds": st[0], "forest_edges": st[1], "entries_read": st[2], "components": st[3],
                          "entries_read_per_round": per_round, "entries_read_over_nnz": round(st[2] / nnz, 3),
                          "GBps_entries_read": round(st[2] * per_entry / t / 1e9, 1),
                          "wcc_mode2_ms": round(t_wcc * 1e3, 3), "wcc_mode2_entries": wst[1],
                          "ratio_to_wcc_mode2": round(t / t_wcc, 2),
                          "note": "host clock around a synchronised call, median of 5 after 2 warm-up; a weighted round reads its "
                                  "live rows twice (min weight, min pair), both counted; bytes per entry read = 4 (column id) + 8 "
                                  "(value) weighted, 4 bool, the gathers of comp[] counted as cache traffic; wcc = fgpu_wcc, "
                                  "wcc_mode 2, on the same pattern"}), flush=True)


def bench_maxflow(ctx, scale, sweep=False):
    """fgpu_maxflow on the directed R-MAT graph with integer capacities 1..100, a fixed hash of (row, col); src = the vertex with
    the most out-entries, sink = the one with the most in-entries among the rest.  For scale, from the same run: one full-pass
    boolean vxm (every frontier bit set) and one fgpu_bfs from src over the same matrix.  sweep: the pulses between two global
    relabels (maxflow_global_every) over 8 .. 1024 instead of the built-in choice."""
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    n = A.nrows
    rp, ci, _ = A.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.repeat(np.arange(n, dtype=np.uint64), deg)
    h = (rows * np.uint64(n) + ci) * np.uint64(0x9E3779B97F4A7C15)   # (mod 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    caps = ((h >> np.uint64(11)) % np.uint64(100) + np.uint64(1)).astype(np.float64)
    Cm = ctx.mat_from_coo(n, n, rows, ci, caps.view(np.uint64))
    src = int(np.argmax(deg))
    indeg = np.bincount(ci.astype(np.int64), minlength=n)
    indeg[src] = -1
    sink = int(np.argmax(indeg))
    del rp, ci, rows, h, caps
    At = A.transpose()
    nnz = A.nvals
    full = np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64)
    if n % 64:
        full[-1] = np.uint64((1 << (n % 64)) - 1)
    t_vxm, _ = timed(ctx, lambda: engine.vxm(ctx, full, None, A, At), reps=5, warm=1)
    level = ctx.host_array(n, np.int32)
    t_bfs, _ = timed(ctx, lambda: engine.bfs(ctx, A, At, src, -1, want_parent=False, level_out=level), reps=5, warm=1)
    # the fixed part of a call: the same matrix from a vertex without any entry — the residual network is built, the labels are
    # set by one global relabel, one empty batch of pulses runs, nothing flows
    lone = np.nonzero((deg == 0) & (indeg == 0))[0]
    t_fixed = None
    if len(lone):
        t_fixed, r0 = timed(ctx, lambda: engine.maxflow(ctx, Cm, int(lone[0]), sink), reps=3, warm=1)
        assert r0[0] == 0.0
    for k in ((8, 16, 32, 64, 128, 256, 1024) if sweep else (0,)):
        ctx.set_option("maxflow_global_every", k)
        t, res = timed(ctx, lambda: engine.maxflow(ctx, Cm, src, sink, stats=True), reps=3, warm=1)
        st = res[4]
        print(json.dumps({"path": "maxflow", "scale": scale, "n": n, "nnz": nnz, "src": src, "sink": sink,
                          "out_degree_src": int(deg[src]), "in_degree_sink": int(indeg[sink]), "maxflow_global_every": k,
                          "ms": round(t * 1e3, 3), "value": res[0], "flow_entries": len(res[1]), "pulses": st[0],
                          "global_relabels": st[1], "residual_arcs": st[2], "pushes": st[3],
                          "Mpushes_per_s": round(st[3] / t / 1e6, 2), "full_vxm_ms": round(t_vxm * 1e3, 3),
                          "bfs_ms": round(t_bfs * 1e3, 3),
                          "ms_call_without_flow": round(t_fixed * 1e3, 3) if t_fixed is not None else None,
                          "note": "host clock around a synchronised call, median of 3 after 1 warm-up (the residual network is "
                                  "built inside every call); call_without_flow = the same call from a vertex without entries: "
                                  "network build + one global relabel + one empty batch of pulses; pushes per second over the whole call; vxm = fgpu_vxm with every "
                                  "frontier bit set, bfs = fgpu_bfs from src, levels only, both median of 5; no outside number "
                                  "exists to compare with"}), flush=True)
    ctx.set_option("maxflow_global_every", 0)


def bench_sssp(ctx, scale, sweep=False):
    """fgpu_sssp on the directed R-MAT graph with weights that are a fixed hash of (row, col), once as integers 1..100 and once
    as uniform doubles in [0, 1); src = the vertex with the most out-entries.  For scale, from the same run: one full-pass
    boolean vxm (every frontier bit set) and one fgpu_bfs from src over the same pattern.  sweep: sssp_delta_log2 over nine
    exponents around the derived one instead of the derived width alone."""
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    n = A.nrows
    rp, ci, _ = A.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.repeat(np.arange(n, dtype=np.uint64), deg)
    h = (rows * np.uint64(n) + ci) * np.uint64(0x9E3779B97F4A7C15)   # (mod 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    weights = {"int_1_100": ((h >> np.uint64(11)) % np.uint64(100) + np.uint64(1)).astype(np.float64),
               "uniform_0_1": (h >> np.uint64(11)).astype(np.float64) / float(1 << 53)}
    src = int(np.argmax(deg))
    del rows, h
    At = A.transpose()
    nnz = A.nvals
    full = np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64)
    if n % 64:
        full[-1] = np.uint64((1 << (n % 64)) - 1)
    t_vxm, _ = timed(ctx, lambda: engine.vxm(ctx, full, None, A, At), reps=5, warm=1)
    level = ctx.host_array(n, np.int32)
    t_bfs, _ = timed(ctx, lambda: engine.bfs(ctx, A, At, src, -1, want_parent=False, level_out=level), reps=5, warm=1)
    out = (ctx.host_array(n, np.float64), ctx.host_array(n, np.int64))
    for name, w in weights.items():
        W = ctx.mat_from_csr(n, n, rp, ci, w.view(np.uint64))
        ctx.set_option("sssp_delta_log2", 4096)
        engine.sssp(ctx, W, src, want_parent=False, out=out)
        auto = ctx.get_option("sssp_last_delta_log2")
        for k in ([auto + d for d in (-4, -3, -2, -1, 0, 1, 2, 3, 4)] if sweep else [4096]):
            ctx.set_option("sssp_delta_log2", k)
            t_dist, _ = timed(ctx, lambda: engine.sssp(ctx, W, src, want_parent=False, out=out), reps=3, warm=1)
            t, (dist, _, st) = timed(ctx, lambda: engine.sssp(ctx, W, src, stats=True, out=out), reps=3, warm=1)
            reached = int(np.isfinite(dist).sum())
            print(json.dumps({"path": "sssp", "scale": scale, "weights": name, "n": n, "nnz": nnz, "src": src,
                              "out_degree_src": int(deg[src]), "sssp_delta_log2": ctx.get_option("sssp_last_delta_log2"),
                              "derived": k == 4096 or k == auto, "ms": round(t * 1e3, 3), "ms_dist_only": round(t_dist * 1e3, 3),
                              "launches": st[0], "popped": st[1], "entries_read": st[2], "deepest": st[3], "reached": reached,
                              "popped_per_reached": round(st[1] / max(reached, 1), 3),
                              "Medges_per_s": round(nnz / t_dist / 1e6, 1), "full_vxm_ms": round(t_vxm * 1e3, 3),
                              "bfs_ms": round(t_bfs * 1e3, 3), "x_bfs": round(t_dist / t_bfs, 2),
                              "note": "host clock around a synchronised call, median of 3 after 1 warm-up; ms = distances + "
                                      "parents, dist_only = parent NULL and stats NULL (no parent search); vxm = fgpu_vxm with "
                                      "every frontier bit set, bfs = fgpu_bfs from src, levels only, both median of 5; x_bfs = "
                                      "dist_only over bfs; no outside number exists to compare with"}), flush=True)
        W.free()
    ctx.set_option("sssp_delta_log2", 4096)


def bench_hops(ctx, scale, host_scale=18):
    """fgpu_sssp_hops on the transposed R-MAT graph with bench_sssp's integer weights (the weight of (u, v) hangs on (v, u)),
    max_hops 3 and 6, beside one fgpu_sssp and one fgpu_bfs from the same vertex; then algo_sp_paths_rows with and without the
    table on the host leg's graph."""
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)
    n = A.nrows
    rp, ci, _ = A.export_csr()
    deg = np.diff(rp.astype(np.int64))
    rows = np.repeat(np.arange(n, dtype=np.uint64), deg)
    h = (rows * np.uint64(n) + ci) * np.uint64(0x9E3779B97F4A7C15)   # (mod 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    w = ((h >> np.uint64(11)) % np.uint64(100) + np.uint64(1)).astype(np.float64)
    Wt = ctx.mat_from_coo(n, n, ci, rows, w.view(np.uint64))   # the transpose, values along
    del h, w
    indeg = np.bincount(ci.astype(np.int64), minlength=n)
    src = int(np.argmax(indeg))
    lone = np.nonzero((deg == 0) & (indeg == 0))[0]
    del rows
    At = A.transpose()
    nnz = A.nvals
    level = ctx.host_array(n, np.int32)
    t_bfs, _ = timed(ctx, lambda: engine.bfs(ctx, At, A, src, -1, want_parent=False, level_out=level), reps=5, warm=1)
    out = (ctx.host_array(n, np.float64), None)
    t_sssp, (dist, _) = timed(ctx, lambda: engine.sssp(ctx, Wt, src, want_parent=False, out=out), reps=3, warm=1)
    reached = int(np.isfinite(dist).sum())
    for hops in (3, 6):
        table = ctx.host_array((hops + 1) * n, np.float64).reshape(hops + 1, n)
        t, (tab, st) = timed(ctx, lambda: engine.sssp_hops(ctx, Wt, src, hops, stats=True, out=table), reps=3, warm=1)
        finite = int(np.isfinite(tab[-1]).sum())   # (before the next call fills the same block)
        t_fixed = None
        if len(lone):
            t_fixed, _ = timed(ctx, lambda: engine.sssp_hops(ctx, Wt, int(lone[0]), hops, out=table), reps=3, warm=1)
        nbytes = (hops + 1) * n * 8
        t_dma = None
        try:   # the same bytes, device to pinned host, on their own
            import torch
            d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            p = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            ts = []
            for k in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p.copy_(d, non_blocking=True)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t_dma = float(np.median(ts[1:]))
            del d, p
        except Exception as e:   # noqa: BLE001
            print(json.dumps({"path": "hops", "dma_probe_failed": str(e)}), flush=True)
        print(json.dumps({"path": "hops", "scale": scale, "weights": "int_1_100", "n": n, "nnz": nnz, "src": src,
                          "in_degree_src": int(indeg[src]), "max_hops": hops, "ms": round(t * 1e3, 3),
                          "table_bytes": nbytes, "ms_dma_alone": round(t_dma * 1e3, 3) if t_dma is not None else None,
                          "ms_less_dma": round((t - t_dma) * 1e3, 3) if t_dma is not None else None,
                          "ms_call_without_search": round(t_fixed * 1e3, 3) if t_fixed is not None else None,
                          "rounds": st[0], "frontier_entries": st[1], "entries_read": st[2], "first_fixed_row": st[3],
                          "finite_in_last_row": finite, "sssp_dist_only_ms": round(t_sssp * 1e3, 3),
                          "sssp_reached": reached, "bfs_ms": round(t_bfs * 1e3, 3), "x_sssp": round(t / t_sssp, 3),
                          "x_bfs": round(t / t_bfs, 2),
                          "note": "host clock around a synchronised call into a pinned table, median of 3 after 1 warm-up; "
                                  "dma_alone = a pinned device-to-host copy of table_bytes by itself, median of 5; "
                                  "call_without_search = the same call from a vertex without entries; sssp = fgpu_sssp, "
                                  "distances only, bfs = fgpu_bfs, levels only, both from src over the same matrix; no outside "
                                  "number exists to compare with"}), flush=True)
    for m in (Wt, At, A):
        m.free()
    # the host call, with and without the table
    from falkordb_amd import host
    hc = host.Context(0)
    B = ctx.mat_rmat(host_scale)
    bn = B.nrows
    brp, bci, _ = B.export_csr()
    bdeg = np.diff(brp.astype(np.int64))
    br = np.repeat(np.arange(bn, dtype=np.uint64), bdeg)
    g = host.Graph(hc, bn)
    ty = g.add_type("KNOWS")
    load_edges(g, ty, br, bci, np.arange(len(bci), dtype=np.uint64))
    g.commit()
    Bt = B.transpose()
    source = int(np.nonzero(bdeg == 8)[0][0])
    lv, _, _ = engine.bfs(ctx, B, Bt, source, -1, want_parent=False)
    far = np.nonzero(lv == 3)[0]
    target = int(far[0]) if len(far) else int(np.nonzero(lv > 0)[0][0])
    for prune in (True, False):
        t0 = time.perf_counter()
        try:
            rows, st = g.algo_sp_paths_rows(source, target, types=["KNOWS"], max_len=4, path_count=0, prune=prune,
                                            max_examined=0 if prune else 300000, stats=True)
            spent = False
        except host.HostError:
            rows, st, spent = [], {"examined": 300000, "pruned_hops": None, "pruned_weight": None, "table_rows": -1}, True
        dt = time.perf_counter() - t0
        print(json.dumps({"path": "hops_host", "scale": host_scale, "n": bn, "nnz": int(len(bci)), "source": source, "target": target,
                          "bfs_level_of_target": int(lv[target]), "max_len": 4, "path_count": 0, "prune": prune,
                          "ms": round(dt * 1e3, 3), "rows": len(rows), "budget_spent": spent, **st,
                          "note": "one call through ctypes, host clock, not repeated; the unpruned walk stops at a budget of "
                                  "300 000 examined successors (budget_spent: its ms and examined are then lower bounds)"}),
              flush=True)
    hc.close()


def bench_asp(ctx, scale, npairs=64):
    """fgpu_shortest_dag between 64 seeded (src, dst) pairs of the R-MAT graph, directed (A, A') and symmetrised (S = A + A' for
    both arguments), two-sided against forward-only, with fgpu_bfs from the same src for scale."""
    def spread(fn, reps=5, warm=1):
        for _ in range(warm):
            r = fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), r

    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    At = A.transpose()
    S = A.merge_pattern(At, None)
    n = A.nrows
    level = ctx.host_array(n, np.int32)
    for graph, M, Mt in (("directed", A, At), ("symmetrised", S, S)):
        rp, _, _ = M.export_csr()
        rpt, _, _ = Mt.export_csr()
        live = np.nonzero((np.diff(rp.astype(np.int64)) > 0) & (np.diff(rpt.astype(np.int64)) > 0))[0]
        rng = np.random.default_rng(0xA5B0 + scale)
        picks = rng.choice(live, size=(npairs, 2))
        rows = []
        for src, dst in picks.tolist():
            ctx.set_option("spdag_sides", 0)
            t2, lo2, hi2, (L, f, _, _, st) = spread(lambda: engine.shortest_dag(ctx, M, Mt, src, dst, stats=True))
            ctx.set_option("spdag_sides", 1)
            t1, lo1, hi1, (L1, f1, _, _, st1) = spread(lambda: engine.shortest_dag(ctx, M, Mt, src, dst, stats=True))
            assert L1 == L and len(f1) == len(f)
            tb, lob, hib, _ = spread(lambda: engine.bfs(ctx, M, Mt, src, -1, want_parent=False, level_out=level), reps=3)
            rows.append((t2, t1, tb))
            print(json.dumps({"path": "asp", "graph": graph, "scale": scale, "src": src, "dst": dst, "L": L, "dag_pairs": len(f),
                              "stats": st, "ms": round(t2, 3), "ms_min_max": [round(lo2, 3), round(hi2, 3)],
                              "forward_only_ms": round(t1, 3), "forward_only_min_max": [round(lo1, 3), round(hi1, 3)],
                              "forward_only_stats": st1, "bfs_ms": round(tb, 3), "bfs_min_max": [round(lob, 3), round(hib, 3)]}),
                  flush=True)
        ctx.set_option("spdag_sides", 0)
        r = np.array(rows)
        q = lambda x: [round(float(v), 3) for v in np.percentile(x, [25, 50, 75])]
        print(json.dumps({"path": "asp_summary", "graph": graph, "scale": scale, "n": n, "nnz": M.nvals, "pairs": npairs,
                          "ms_q25_q50_q75": q(r[:, 0]), "forward_only_ms_q25_q50_q75": q(r[:, 1]), "bfs_ms_q25_q50_q75": q(r[:, 2]),
                          "two_sided_over_forward_only_q25_q50_q75": q(r[:, 0] / r[:, 1]),
                          "two_sided_over_bfs_q25_q50_q75": q(r[:, 0] / r[:, 2]),
                          "note": "host clock around a synchronised call; per pair the median of 5 after 1 warm-up (bfs: of 3), the "
                                  "summary gives the quartiles over the 64 pairs; bfs = fgpu_bfs from src, levels only, on its cached "
                                  "plan; no outside number exists to compare with"}), flush=True)
    S.free()
    At.free()
    A.free()


def bench_asp_batch(ctx, scale, npairs=64, nbig=1024, host_scale=18):
    """fgpu_shortest_dag_batch against the loop of single calls over the same pairs, same process, same handles"""
    def spread(fn, reps=5, warm=1):
        for _ in range(warm):
            r = fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), r

    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    At = A.transpose()
    S = A.merge_pattern(At, None)
    n = A.nrows
    ctx.set_option("spdag_sides", 0)
    for graph, M, Mt in (("directed", A, At), ("symmetrised", S, S)):
        rp, _, _ = M.export_csr()
        rpt, _, _ = Mt.export_csr()
        live = np.nonzero((np.diff(rp.astype(np.int64)) > 0) & (np.diff(rpt.astype(np.int64)) > 0))[0]
        rng = np.random.default_rng(0xA5B0 + scale)
        picks = rng.choice(live, size=(npairs, 2))           # the asp leg's pairs
        big = np.random.default_rng(0xB16 + scale).choice(live, size=(nbig, 2))
        src, dst = picks[:, 0].tolist(), picks[:, 1].tolist()
        ta, loa, hia, one = spread(lambda: [engine.shortest_dag(ctx, M, Mt, s, d, stats=True) for s, d in zip(src, dst)])
        tb, lob, hib, bat = spread(lambda: engine.shortest_dag_batch(ctx, M, Mt, src, dst, stats=True))
        equal = all(x[0] == y[0] and x[4] == y[4] and all(np.array_equal(p, q) for p, q in zip(x[1:4], y[1:4]))
                    for x, y in zip(one, bat))
        tc, loc, hic, bigr = spread(lambda: engine.shortest_dag_batch(ctx, M, Mt, big[:, 0], big[:, 1], stats=True))
        scanned = lambda rs: int(sum(r[4][4] + r[4][5] for r in rs))
        print(json.dumps({"path": "asp_batch", "graph": graph, "scale": scale, "n": n, "nnz": M.nvals, "pairs": npairs,
                          "a_loop_ms_per_query": round(ta / npairs, 4), "a_loop_ms_min_max": [round(loa, 3), round(hia, 3)],
                          "b_batch_ms_per_query": round(tb / npairs, 4), "b_batch_ms_min_max": [round(lob, 3), round(hib, 3)],
                          "a_over_b": round(ta / tb, 2), "b_equals_a": bool(equal), "entries_scanned_64": scanned(bat),
                          "found_64": int(sum(r[0] > 0 for r in bat)), "dag_pairs_64": int(sum(len(r[1]) for r in bat)),
                          "c_pairs": nbig, "c_batch_ms_per_query": round(tc / nbig, 4), "c_batch_ms_min_max": [round(loc, 3), round(hic, 3)],
                          "c_entries_scanned": scanned(bigr), "c_found": int(sum(r[0] > 0 for r in bigr)),
                          "c_dag_pairs": int(sum(len(r[1]) for r in bigr)),
                          "note": "host clock around synchronised calls in one process, median of 5 after 1 warm-up; (a) 64 "
                                  "fgpu_shortest_dag calls in a loop, (b) one fgpu_shortest_dag_batch of the same 64, (c) one of 1024 "
                                  "seeded pairs at slots = 0; stats on, transpose given, spdag_sides 0"}), flush=True)
    S.free()
    At.free()
    A.free()
    # the host operator on the host leg's graph: one batch of 64 rows against the per-row loop, the operator's own clock
    from falkordb_amd import host
    hc = host.Context(0)
    B = ctx.mat_rmat(host_scale)
    bn = B.nrows
    brp, bci, _ = B.export_csr()
    bdeg = np.diff(brp.astype(np.int64))
    g = host.Graph(hc, bn)
    ty = g.add_type("KNOWS")
    load_edges(g, ty, np.repeat(np.arange(bn, dtype=np.uint64), bdeg), bci, np.arange(len(bci), dtype=np.uint64))
    g.commit()
    B.free()
    live = np.nonzero(bdeg > 0)[0]
    rows = np.random.default_rng(0xA5B0 + host_scale).choice(live, size=(npairs, 2))
    loop_ms, batch_ms = [], []
    for rep in range(4):   # (the first repetition warms both up)
        t = 0
        per_row = []
        for s, d in rows.tolist():
            per_row.append(g.all_shortest_paths(s, d, types=["KNOWS"], limit=16))
            t += g.L.fh_last_op_ns() / 1e9
        got = g.all_shortest_paths_batch(rows[:, 0], rows[:, 1], types=["KNOWS"], limit=16)
        if rep:
            loop_ms.append(t * 1e3)
            batch_ms.append(g.L.fh_last_op_ns() / 1e9 * 1e3)
    print(json.dumps({"path": "asp_batch_host", "scale": host_scale, "n": bn, "nnz": int(len(bci)), "rows": npairs, "limit": 16,
                      "loop_ms_per_row": round(float(np.median(loop_ms)) / npairs, 4),
                      "batch_ms_per_row": round(float(np.median(batch_ms)) / npairs, 4), "equal": got == per_row,
                      "note": "fh_last_op_ns around the operator, median of 3 after 1 warm-up; the loop builds the adjacency per row"}),
          flush=True)
    hc.close()


def bench_shortest_path(ctx, scale, npairs=64, nbig=1024, host_scale=18):
    """fgpu_shortest_path_batch: one batch against a loop of one-query calls and against fgpu_shortest_dag_batch on the same
    pairs, same process, same handles; then the host function's batch against its per-row loop"""
    def spread(fn, reps=5, warm=1):
        for _ in range(warm):
            r = fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), r

    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    At = A.transpose()
    S = A.merge_pattern(At, None)
    n = A.nrows
    ctx.set_option("spdag_sides", 0)
    for graph, M, Mt in (("directed", A, At), ("symmetrised", S, S)):
        rp, _, _ = M.export_csr()
        rpt, _, _ = Mt.export_csr()
        live = np.nonzero((np.diff(rp.astype(np.int64)) > 0) & (np.diff(rpt.astype(np.int64)) > 0))[0]
        picks = np.random.default_rng(0xA5B0 + scale).choice(live, size=(npairs, 2))           # the asp leg's pairs
        big = np.random.default_rng(0xB16 + scale).choice(live, size=(nbig, 2))                # the asp_batch leg's
        src, dst = picks[:, 0].tolist(), picks[:, 1].tolist()
        ta, loa, hia, one = spread(lambda: [engine.shortest_path_batch(ctx, M, Mt, [s], [d], stats=True)[0] for s, d in zip(src, dst)])
        tb, lob, hib, bat = spread(lambda: engine.shortest_path_batch(ctx, M, Mt, src, dst, stats=True))
        equal = all((x[0] is None) == (y[0] is None) and (x[0] is None or np.array_equal(x[0], y[0])) and x[1] == y[1]
                    for x, y in zip(one, bat))
        tc, loc, hic, bigr = spread(lambda: engine.shortest_path_batch(ctx, M, Mt, big[:, 0], big[:, 1], stats=True))
        td, lod, hid, dag = spread(lambda: engine.shortest_dag_batch(ctx, M, Mt, src, dst, stats=True))
        te, loe, hie, dagbig = spread(lambda: engine.shortest_dag_batch(ctx, M, Mt, big[:, 0], big[:, 1], stats=True))
        same_len = all((p is None and r[0] < 0) or (p is not None and len(p) - 1 == r[0]) for (p, _), r in zip(bat, dag))
        walked = lambda rs: int(sum(st[4] for _, st in rs))
        rounds = lambda rs: int(max(st[0] + st[1] for _, st in rs))
        print(json.dumps({"path": "shortest_path", "graph": graph, "scale": scale, "n": n, "nnz": M.nvals, "pairs": npairs,
                          "a_loop_ms_per_query": round(ta / npairs, 4), "a_loop_ms_min_max": [round(loa, 3), round(hia, 3)],
                          "b_batch_ms_per_query": round(tb / npairs, 4), "b_batch_ms_min_max": [round(lob, 3), round(hib, 3)],
                          "a_over_b": round(ta / tb, 2), "b_equals_a": bool(equal), "entries_walked_64": walked(bat),
                          "found_64": int(sum(p is not None for p, _ in bat)), "rounds_64": rounds(bat),
                          "c_pairs": nbig, "c_batch_ms_per_query": round(tc / nbig, 4), "c_batch_ms_min_max": [round(loc, 3), round(hic, 3)],
                          "c_entries_walked": walked(bigr), "c_found": int(sum(p is not None for p, _ in bigr)),
                          "d_dag_batch_ms_per_query": round(td / npairs, 4), "d_dag_batch_ms_min_max": [round(lod, 3), round(hid, 3)],
                          "d_lengths_equal_b": bool(same_len), "d_entries_scanned_64": int(sum(r[4][4] + r[4][5] for r in dag)),
                          "e_dag_batch_1024_ms_per_query": round(te / nbig, 4), "e_min_max": [round(loe, 3), round(hie, 3)],
                          "b_over_d": round(tb / td, 2), "c_over_e": round(tc / te, 2),
                          "note": "host clock around synchronised calls in one process, median of 5 after 1 warm-up; (a) 64 "
                                  "fgpu_shortest_path_batch calls of one query in a loop, (b) one call of the same 64, (c) one of 1024 "
                                  "seeded pairs at slots = 0, (d) / (e) fgpu_shortest_dag_batch on the pairs of (b) / (c); stats on, "
                                  "backward pattern given; rounds_64 = the most levels any query of (b) ran"}), flush=True)
    S.free()
    At.free()
    A.free()
    # the host function on the host leg's graph: one batch of 64 rows against the per-row loop, the function's own clock
    from falkordb_amd import host
    hc = host.Context(0)
    B = ctx.mat_rmat(host_scale)
    bn = B.nrows
    brp, bci, _ = B.export_csr()
    bdeg = np.diff(brp.astype(np.int64))
    g = host.Graph(hc, bn)
    ty = g.add_type("KNOWS")
    load_edges(g, ty, np.repeat(np.arange(bn, dtype=np.uint64), bdeg), bci, np.arange(len(bci), dtype=np.uint64))
    g.commit()
    B.free()
    live = np.nonzero(bdeg > 0)[0]
    rows = np.random.default_rng(0xA5B0 + host_scale).choice(live, size=(npairs, 2)).tolist()
    batch_ms = []
    for rep in range(4):   # (the first repetition warms up)
        got = g.shortest_path_batch([s for s, _ in rows], [d for _, d in rows], types=["KNOWS"])
        if rep:
            batch_ms.append(g.L.fh_last_op_ns() / 1e9 * 1e3)
    t, per_row, t0 = 0, [], time.perf_counter()
    for s, d in rows:      # eval_row fetches one matrix row per iterator call: once through, up to a deadline
        per_row.append(g.shortest_path(s, d, types=["KNOWS"]))
        t += g.L.fh_last_op_ns() / 1e9
        if time.perf_counter() - t0 > 90:
            break
    print(json.dumps({"path": "shortest_path_host", "scale": host_scale, "n": bn, "nnz": int(len(bci)), "rows": npairs,
                      "loop_rows_timed": len(per_row), "loop_ms_per_row": round(t * 1e3 / len(per_row), 4),
                      "batch_ms_per_row": round(float(np.median(batch_ms)) / npairs, 4), "equal": got[:len(per_row)] == per_row,
                      "found": int(sum(r is not None for r in got)),
                      "note": "fh_last_op_ns around the function; the batch: median of 3 after 1 warm-up; the loop is eval_row, "
                              "which walks the versioned matrices' rows one iterator call at a time: once through, cut off "
                              "after 90 s (loop_rows_timed)"}), flush=True)
    hc.close()


def bench_betweenness(ctx, scale):
    from falkordb_amd import host
    A = ctx.mat_rmat(scale, 16, 0x5EED1234 + scale)          # bench.py's graph of that scale
    At = A.transpose()
    n, nnz = A.nrows, A.nvals
    out = ctx.host_array(n, np.float64)
    level = ctx.host_array(n, np.int32)
    for label, src in (("seed0_16", host.betweenness_sources(n, 16, 0)), ("lcg_16", host.betweenness_sources(n, 16, 10)),
                       ("lcg_256", host.betweenness_sources(n, 256, 10))):
        tb, _ = timed(ctx, lambda: [engine.bfs(ctx, A, At, int(s), -1, want_parent=False, level_out=level) for s in src],
                      reps=5, warm=1)
        for d in (0, 1, 2):
            ctx.set_option("bc_direction", d)
            t, (_, st) = timed(ctx, lambda: engine.betweenness(ctx, A, src, At, stats=True, out=out), reps=10, warm=2)
            width = 16 if len(src) <= 16 else 64
            bound_ms = st[0] * (2 * (4 * nnz + 4 * (n + 1)) + 2 * n * width * 20) / 8e12 * 1e3
            print(json.dumps({"path": "betweenness", "scale": scale, "sources": label, "nsrc": len(src), "bc_direction": d,
                              "n": n, "nnz": nnz, "ms": round(t * 1e3, 3), "batches": st[0], "forward_levels": st[1],
                              "entries_read": st[2], "deepest": st[3], "bound_ms": round(bound_ms, 4),
                              "bfs_x_sources_ms": round(tb * 1e3, 3),
                              "note": "host clock around a synchronised call, median of 10 after 2 warm-up; bfs = fgpu_bfs "
                                      "once per source, median of 5; bound = per batch 2 (4 nnz + 4 (n + 1)) + 2 n B 20 "
                                      "bytes at 8 TB/s"}), flush=True)
    ctx.set_option("bc_direction", 0)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    if what in ("merge", "all"):
        c = engine.Context(0)
        bench_merge(c, scale or 22)
        c.close()
    if what in ("expand", "all"):
        import os
        world, rank, dev = int(os.environ.get("WORLD_SIZE", "1")), 0, "cpu"
        if world > 1:    # python -m torch.distributed.run --nproc-per-node N tools/bench_paths.py expand 24
            import torch
            import torch.distributed as td
            rank = int(os.environ["RANK"])
            local = int(os.environ.get("LOCAL_RANK", rank))
            torch.cuda.set_device(local)
            dev = torch.device("cuda", local)
            td.init_process_group("nccl", device_id=dev)
            c = engine.Context(local)
        else:
            c = engine.Context(0)
        bench_expand(c, scale or 24, rank=rank, nranks=world, device=dev)
        c.close()
        if world > 1:
            td.destroy_process_group()
        if what == "expand":
            sys.exit(0)
    if what in ("reach", "all"):
        c = engine.Context(0)
        bench_reach(c, scale or 19)
        c.close()
    if what in ("pagerank", "all"):
        c = engine.Context(0)
        bench_pagerank(c, scale or 22)
        c.close()
    if what in ("wcc", "all"):
        c = engine.Context(0)
        for sc in ([scale] if scale else [22, 24]):
            bench_wcc(c, sc)
        c.close()
    if what in ("cdlp", "all"):
        c = engine.Context(0)
        for sc in ([scale] if scale else [22, 24]):
            bench_cdlp(c, sc)
        c.close()
    if what in ("harmonic", "all"):
        c = engine.Context(0)
        bench_harmonic(c, scale if scale else 22)
        c.close()
    if what in ("msf", "all"):
        c = engine.Context(0)
        bench_msf(c, scale if scale else 22)
        c.close()
    if what in ("maxflow", "maxflow_sweep", "all"):
        c = engine.Context(0)
        bench_maxflow(c, scale if scale else 22, sweep=what == "maxflow_sweep")
        c.close()
    if what in ("sssp", "sssp_sweep", "all"):
        c = engine.Context(0)
        bench_sssp(c, scale if scale else 22, sweep=what == "sssp_sweep")
        c.close()
    if what in ("hops", "all"):
        c = engine.Context(0)
        bench_hops(c, scale if scale else 22)
        c.close()
    if what in ("asp", "all"):
        c = engine.Context(0)
        bench_asp(c, scale if scale else 22)
        c.close()
    if what in ("asp_batch", "all"):
        c = engine.Context(0)
        bench_asp_batch(c, scale if scale else 22)
        c.close()
    if what in ("shortest_path", "all"):
        c = engine.Context(0)
        bench_shortest_path(c, scale if scale else 22)
        c.close()
    if what in ("betweenness", "all"):
        c = engine.Context(0)
        for sc in ([scale] if scale else [22, 24]):
            bench_betweenness(c, sc)
        c.close()
    if what in ("host", "all"):
        bench_host(scale or 18)
    if what == "load":                           # (minutes of edge-by-edge loading: not part of `all`)
        bench_load(*(((scale,), 0) if scale else ()))
    if what == "detach":                         # (edge-by-edge deletes up to their deadlines: not part of `all`)
        bench_detach(*(((), scale, 0) if scale else ()))
    if what == "edel":                           # (edge-by-edge deletes up to their deadlines: not part of `all`)
        bench_edel(*(((scale,), 0) if scale else ()))
    if what == "edges":                          # (the per-row path up to its deadlines: not part of `all`)
        bench_edges(*(((scale,),) if scale else ()))
    if what == "degrees":                        # (the eval_row loop up to its deadline: not part of `all`)
        bench_degrees(*(((scale,), 18, 0) if scale else ()))
    if what == "varlen_batch":                   # (the loop of expand_row up to its deadlines: not part of `all`)
        bench_varlen(*((scale,) if scale else ()))
    if what == "append":                         # (seconds of edge-by-edge inserts per twin: not part of `all`)
        bench_append(*(((scale,), 0) if scale else ()))
