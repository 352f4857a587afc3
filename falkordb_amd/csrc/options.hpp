// options.hpp — the engine options and the one table behind fgpu_set_option / fgpu_get_option.
// Plain C++17: no HIP, nothing of common.hpp, so the table is testable on the host (tests/host/options_check.cpp).
// A new option is a field of fgpu_options, a row of OPTIONS below and a line in include/fgpu.h.
#pragma once
#include <stdint.h>
#include <string.h>

struct fgpu_options {  // fgpu_set_option
    int tiled_u = 8;           // items in flight per wavefront of the tiled kernel (8 KiB of entries per wave)
    int tiled_nt = 0;          // nontemporal entry loads
    int tiled_threads = 1024;  // its workgroup size
    int tiled_wgs = 0;         // its grid (0 = one workgroup per CU)
    int expand_mode = 0;       // 0 auto, 1 sorted-CSR products only, 2 bit-parallel from the first hop
    int expand_row_groups = 1; // sparse mid-chain pull: a wavefront per 32-row group (0 = a wavefront per row item)
    int expand_fuse_count = 1; // fgpu_expand_count: the last bit-parallel hop counts its rows in place (0 = separate count pass)
    int expand_bits_ratio = 28; // fgpu_expand, expand_mode 0: a hop goes to bit form when its traversed edges T exceed nnz / ratio
    int blocked_variant = 0;   // blocked.hip kernel variant (trips in flight / workgroups per CU), see blocked_mxv
    int tiled_layout = 0;      // full-pass pull layout: 0 = pick by size, 1 = LDS x tiles + global atomics (tiled.hip), 2 = x tile
                               // and output window both in LDS (blocked.hip)
    int bfs_wgs_per_cu = 6;    // grid of the fused BFS level kernel, workgroups per CU
    int bfs_tiny = 2;          // consecutive tiny BFS levels in one single-workgroup launch (bfs_tiny_kernel): 0 off, 1 on,
                               // 2 = when the plan's previous search took more than 12 levels
    int bfs_hub_first = 1;     // pull levels read A' rows reordered hub-first (bfs.hip ensure_pull_order)
    int bfs_alive_rule = 1;    // push <-> pull rule of the fused BFS: the unvisited share is taken over the vertices that have an in-edge
                               // (0 = over all vertices, rounds 1-5; A/B)
    int bfs_pb = 1;            // heavy push levels by propagation blocking (bfs.hip bfs_pb_*): the frontier's edges are binned by
                               // destination window, a workgroup per window marks its discoveries in LDS — no global atomic per
                               // edge.  0 off, 1 for plans of at least 2^24 vertices (a heavy push level of a smaller graph is a
                               // few tens of microseconds: the four extra launches cost more), 2 for every single-rank plan
    long long bfs_pb_min_edges = 2ll << 20;   // ... a push level with at least this many edges to examine goes that way
    int bfs_prof_split = 0;    // profiled BFS pass launches the <.., 1|2> twins that name a level push / pull (PMC passes)
    int merge_items = 1;       // Delta merge scatter: 1 = shifted copy by 2048-entry items with the dp insertion positions as events
                               // (merge.hip), 0 = the per-word / per-entry scatter (A/B)
    int merge_mode = 0;        // Delta merge: 0 entry-parallel (merge.hip), 1 one wavefront per row (pattern only)
    int dist_timing = 0;       // fgpu_bfs_dist_run records HIP events around every level kernel and exchange (fgpu_bfs_dist_times)
    int dist_collective = 0;   // frontier exchange of the in-library multi-GPU BFS: 0 grouped ncclSend/ncclRecv
                               // (all-gather-v, direct peer-to-peer over xGMI), 1 one ncclBroadcast per rank in a group
    int dist_force_self = 0;   // TEST ONLY: a communicator of one rank still issues the grouped self send / recv, broadcast and
                               // all-reduce of a multi-rank exchange (dist.hip) — the code path on the real librccl of a 1-GPU box
    int dist_test_delay_us = 0; // TEST ONLY: fgpu_bfs_dist_run puts a kernel spinning this many microseconds behind every level kernel of
                               // THIS context's rank (a peer that finishes its levels late; tests/test_gpu_dist.py)
    int transpose_mode = 0;    // pattern transpose / COO build: 0 counting sort (form picked by key space), 1 COO rebuild through the sorter (A/B), 2 LDS-staged levels, 3 two levels
    int lds_limit = 0;         // usable LDS bytes per workgroup (filled by fgpu_init)
    int expand_compact = 1;    // fgpu_expand*: source rows that are empty after the CSR hops (sources without out-edges: half of an
                               // R-MAT batch) are dropped before the chain goes to bits when that halves the row width (0 = keep; A/B)
    int pagerank_parts = 1;    // PageRank SpMV: 1 = A' in 8 column ranges, range k gathered by XCD k out of its own L2 (when the score
                               // vector exceeds one L2), 2 = always, 0 = the one-pass pull over the whole vector (A/B)
    int expand_first_hop = 1;  // fgpu_expand*: a clean first hop from one-entry rows copies the source rows (0 = the general product; A/B)
    int expand_xcd = 1;        // dense count hop of the bit-parallel chain: 1 = the rows of X are gathered by the XCD that owns their
                               // partition, partial rows folded per vertex (bitpart.hip), 0 = every workgroup gathers from all of X (A/B)
    int expand_xcd_relabel = 1; // ... and the state it reads is laid out hot-first per partition by the hop that produces it (0 = vertex order; A/B)
    int expand_xcd_min_mb = 32; // ... when the bit state holds at least this many MiB (8 L2s of 4 MiB; below that the plain pull)
    int expand_xp_direct = 1;   // ... 1 = a (partition, row) run of ONE entry leaves the stream: the fold reads that row of X itself
                               // instead of a partial row the stream kernel copied out of it (bitpart.hip), 0 = every run is streamed (A/B)
    int expand_xp_fold = 1;     // ... the fold of the partial rows: 1 = the index work once per row and one load per piece that exists
                               // (xp_fold_pieces_kernel), 0 = a slot per row and step, 8 loads each, most of them the zero row (A/B)
    int expand_xp_fold_min_words = 8; // ... the piece fold runs on bit rows of at least this many 64-bit words, narrower rows keep the slot
                               // fold: at 2 and 4 words the piece fold is 30 us per launch SLOWER (its fixed work per group outweighs
                               // the few look-ups of a narrow row), at 8 it is 24 us faster, at 16 103 us (profiles/NOTES_r12.md section 3.5)
    int expand_xp_dense = 1;    // ... the fold's groups: 1 = 64 consecutive RANKS among the rows that have an in-edge (at RMAT-22 48 % of
                               // the rows: half the groups, no lane on a row that cannot hold a piece), 0 = 64 consecutive vertex ids (A/B)
    int expand_scan_min = 2048; // fgpu_expand_count: a call with more source rows than this is a WHOLE-FRONTIER call (spgemm.hip
                               // expand_count_scan): live rows filtered and compacted on the device, cut into passes (0 = never)
    int expand_scan_rows = 1024; // ... live rows per pass: 1024 = 16 words = one 128-byte line per vertex of the bit state
    int expand_scan_lanes = 3;  // ... lanes (calling thread + workers, a stream and pool each) the passes are dealt to
    int expand_records = 1;     // sparse mid-chain pull: rows of X with <= 4 bits are read as 8-byte records of source indices, a lane
                               // per live entry (bitexpand.hip bp_records_kernel; 0 = every live entry gathers the whole row; A/B)
    int expand_nt = 1;          // XCD-partitioned count hop, streaming hints (bit mask): 1 = the partial rows leave the stream kernel with
                               // non-temporal stores (1 GB per pass that would otherwise displace the partition's hot rows of X from its L2:
                               // stream kernel 824 -> 771 us at RMAT-22, no change at RMAT-26), 2 = its column-id stream is read non-temporal,
                               // 4 = the fold reads the partial rows non-temporal (2, 4: no effect, off; profiles/NOTES_r06.md section 7)
    int expand_emit_sort = 1;   // bit state -> CSR: 2 = (row, vertex) pairs in vertex order + the LDS-staged stable sort by row, 0 = the
                               // ballot transpose of rounds 3-5 (bp_rows_kernel), 1 = pairs + sort unless the count pass finds more
                               // than 8 entries per vertex (a dense result: the ballot transpose is 4 x cheaper there)
    int pinned_results = 1;    // result arrays >= 256 KiB come from the context's pinned-host pool and are filled by DMA (0 = the
                               // caller's allocator / malloc + staged copies, the round-3 path; A/B)
    int pinned_pool_mb = 4096; // pinned blocks kept for reuse after fgpu_free (beyond it they go back to the OS)
    int wcc_mode = 0;          // fgpu_wcc: 0 auto (Afforest from 4096 vertices), 1 Afforest with sampling and skip, 2 one full link
                               // pass over every entry of A (wcc.hip)
    int bc_batch = 0;          // fgpu_betweenness: sources per batch, 0 auto (16 / 32 / 64 by nsrc, halved to fit free memory), 1-64 forced
    int maxflow_global_every = 0;   // fgpu_maxflow: pulses between two global relabels (0 = MF_GLOBAL_EVERY of maxflow.hip; A/B)
    int bc_direction = 0;      // fgpu_betweenness forward levels: 0 auto (push / pull by entries to read), 1 push over A, 2 pull over At
    int sssp_delta_log2 = 4096; // fgpu_sssp: the bucket width is 2^value, SSSP_DELTA_AUTO = derived on the device from the mean finite
                               // weight and the mean degree (sssp.hip).  Handled in ctx.hip, not a row below: an exponent or auto: no row kind fits
    int expand_group_items = 1; // sparse mid-chain pull through records, the rows of <= 256 entries: 0 = a wavefront per 32-row group
                               // derives the cut of its rows in every pass (rowptr -> prefix scan -> column ids), 1 = a wavefront per
                               // ITEM of the packed stream built once per snapshot (bitexpand.hip bp_group_items: <= 32 whole rows,
                               // <= 256 entries, the row of an entry in bits 27..31 of its column word; A/B: 277 -> 228 us a launch at
                               // RMAT-22, profiles/NOTES_r17.md)
    int expand_xp_lookahead = 1; // XCD-partitioned count hop, stream kernel: 1 = the loads a chunk's last iteration issues ahead are the first
                               // two trips of the wavefront's NEXT chunk, 0 = they repeat the chunk's last entry and every chunk opens its own
                               // pipeline (bitpart.hip xp_stream_kernel; A/B, profiles/NOTES_r18.md)
    int expand_xp_cut = 1;      // ... its chunk table: 1 = every chunk but a partition's last holds a multiple of 128 entries, two whole
                               // trips of the stream kernel (bitpart.hip xp_cut_cells), 0 = the key cut (entry + 8 x run) / 768
    int expand_xp_stream_wgs = 0; // ... at most this many workgroups of the stream kernel per partition, 0 = as many as the chunks and the
                               // CUs allow (tests: every wavefront walks many chunks of a small graph; A/B)
    int spdag_sides = 0;        // fgpu_shortest_dag: which ball grows.  0 = the side whose frontier has fewer entries to scan (ties
                               // forward), 1 = forward only, 2 = backward only, 3 = strict alternation starting forward.  Every
                               // setting returns the same length and pairs, only the stats differ (spdag.hip; the tests hold the
                               // two-sided search to the one-sided ones)
    int degree_window_rows = 1 << 24; // fgpu_node_degrees: positions per window (degrees.hip): a call walks its batch, or the whole
                               // graph, in windows of at most this many rows, so the segment and entry spaces of one window stay
                               // inside 32 bits.  Handled in ctx.hip like sssp_delta_log2, not a row below
};
constexpr int SSSP_DELTA_AUTO = 4096, SSSP_DELTA_MIN = -1074, SSSP_DELTA_MAX = 1023;
// the values "degree_window_rows" accepts: range-checked in ctx.hip
constexpr int DEGREE_WINDOW_MIN = 64, DEGREE_WINDOW_MAX = 1 << 24;

namespace fgpu {

// ---- the option table --------------------------------------------------------------
// One row per settable option, in the order of the struct.  What a row accepts:
//   OPT_BOOL   any value, stored as value != 0
//   OPT_RANGE  lo <= value <= hi
//   OPT_POW2   lo <= value <= hi and a power of two
// Not in the table: lds_limit (filled by fgpu_init, not settable), "transpose_wb" (process-wide, no field), sssp_delta_log2 and
// degree_window_rows: ctx.hip.
enum OptKind { OPT_BOOL, OPT_RANGE, OPT_POW2 };

struct OptRow {
    const char* name;
    int fgpu_options::*i32;          // the field ...
    long long fgpu_options::*i64;    // ... or the one 64-bit field (bfs_pb_min_edges); exactly one of the two is set
    OptKind kind;
    int64_t lo, hi;
};

#define FGPU_OPT(field, kind, lo, hi) {#field, &fgpu_options::field, nullptr, kind, lo, hi}
#define FGPU_OPT64(field, kind, lo, hi) {#field, nullptr, &fgpu_options::field, kind, lo, hi}
inline constexpr OptRow OPTIONS[] = {
    FGPU_OPT(tiled_u, OPT_POW2, 1, 8),
    FGPU_OPT(tiled_nt, OPT_BOOL, 0, 1),
    FGPU_OPT(tiled_threads, OPT_POW2, 256, 1024),
    FGPU_OPT(tiled_wgs, OPT_RANGE, 0, 65536),
    FGPU_OPT(expand_mode, OPT_RANGE, 0, 2),
    FGPU_OPT(expand_row_groups, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_fuse_count, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_bits_ratio, OPT_RANGE, 1, 1024),
    FGPU_OPT(blocked_variant, OPT_RANGE, 0, 3),
    FGPU_OPT(tiled_layout, OPT_RANGE, 0, 2),
    FGPU_OPT(bfs_wgs_per_cu, OPT_RANGE, 1, 64),
    FGPU_OPT(bfs_tiny, OPT_RANGE, 0, 2),
    FGPU_OPT(bfs_hub_first, OPT_BOOL, 0, 1),
    FGPU_OPT(bfs_alive_rule, OPT_BOOL, 0, 1),
    FGPU_OPT(bfs_pb, OPT_RANGE, 0, 2),
    FGPU_OPT64(bfs_pb_min_edges, OPT_RANGE, 1, INT64_MAX),
    FGPU_OPT(bfs_prof_split, OPT_BOOL, 0, 1),
    FGPU_OPT(merge_items, OPT_BOOL, 0, 1),
    FGPU_OPT(merge_mode, OPT_RANGE, 0, 2),
    FGPU_OPT(dist_timing, OPT_BOOL, 0, 1),
    FGPU_OPT(dist_collective, OPT_RANGE, 0, 1),
    FGPU_OPT(dist_force_self, OPT_BOOL, 0, 1),
    FGPU_OPT(dist_test_delay_us, OPT_RANGE, 0, 100000),
    FGPU_OPT(transpose_mode, OPT_RANGE, 0, 3),
    FGPU_OPT(expand_compact, OPT_BOOL, 0, 1),
    FGPU_OPT(pagerank_parts, OPT_RANGE, 0, 2),
    FGPU_OPT(expand_first_hop, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_xcd, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_xcd_relabel, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_xcd_min_mb, OPT_RANGE, 0, 1 << 20),
    FGPU_OPT(expand_xp_direct, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_xp_fold, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_xp_fold_min_words, OPT_POW2, 2, 32),
    FGPU_OPT(expand_xp_dense, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_scan_min, OPT_RANGE, 0, INT32_MAX),
    FGPU_OPT(expand_scan_rows, OPT_POW2, 64, 4096),
    FGPU_OPT(expand_scan_lanes, OPT_RANGE, 1, 16),
    FGPU_OPT(expand_records, OPT_BOOL, 0, 1),
    FGPU_OPT(expand_nt, OPT_RANGE, 0, 7),
    FGPU_OPT(expand_emit_sort, OPT_RANGE, 0, 2),
    FGPU_OPT(pinned_results, OPT_BOOL, 0, 1),
    FGPU_OPT(pinned_pool_mb, OPT_RANGE, 0, 1 << 20),
    FGPU_OPT(wcc_mode, OPT_RANGE, 0, 2),
    FGPU_OPT(bc_batch, OPT_RANGE, 0, 64),
    FGPU_OPT(maxflow_global_every, OPT_RANGE, 0, 1 << 20),
    FGPU_OPT(bc_direction, OPT_RANGE, 0, 2),
    FGPU_OPT(expand_group_items, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_xp_lookahead, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_xp_cut, OPT_RANGE, 0, 1),
    FGPU_OPT(expand_xp_stream_wgs, OPT_RANGE, 0, 65536),
    FGPU_OPT(spdag_sides, OPT_RANGE, 0, 3),
};
#undef FGPU_OPT
#undef FGPU_OPT64

inline const OptRow* opt_find(const char* name) {
    for (const OptRow& r : OPTIONS)
        if (!strcmp(r.name, name)) return &r;
    return nullptr;
}

inline bool opt_accepts(const OptRow& r, int64_t v) {
    if (r.kind == OPT_BOOL) return true;
    if (v < r.lo || v > r.hi) return false;
    return r.kind != OPT_POW2 || (v & (v - 1)) == 0;   // lo >= 1 on every OPT_POW2 row
}

// `v` is a value opt_accepts(r, v) passed
inline void opt_store(fgpu_options& o, const OptRow& r, int64_t v) {
    if (r.kind == OPT_BOOL) v = v != 0;
    if (r.i64) o.*r.i64 = v;
    else o.*r.i32 = (int)v;
}

inline int64_t opt_load(const fgpu_options& o, const OptRow& r) {
    return r.i64 ? (int64_t)(o.*r.i64) : (int64_t)(o.*r.i32);
}

}  // namespace fgpu
