/*
 * fgpu.h — C ABI of the MI355X-native traversal engine (device tier).
 *
 * This is the drop-in boundary for FalkorDB's sparse-linear-algebra hot path.
 * In the reference the boundary is the `extern "C"` GraphBLAS/LAGraph symbol set
 * bound by bindgen (graph/src/graph/graphblas/mod.rs:42-79) and consumed only
 * through `Matrix<T>` (graph/src/graph/graphblas/matrix.rs).  Every entry point
 * below names the reference call it replaces (file:line relative to
 * /root/reference).  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add beside graphblas/mod.rs.
 *
 * Conventions (mirroring SURVEY.md §8b):
 *  - plain pointers and sizes only; no C++ / torch types cross this boundary;
 *  - every call returns an fgpu_info (values 0/1/-2/-3/-102/-105 mirror
 *    GrB_Info, graphblas/mod.rs:274-296); never aborts, never throws;
 *  - fgpu_last_error() returns a thread-local message for the last failure;
 *  - an fgpu_mat is an IMMUTABLE device-resident snapshot (the committed,
 *    `wait()`ed state of a reference Matrix: CSR, sorted unique columns per
 *    row, pattern-only for BOOL, +u64 values for UINT64 tensors);
 *  - node ids must fit in 32 bits (the reference's Tensor::compound_key makes
 *    the same demand, tensor.rs:154-163) and nnz per matrix must be < 2^32;
 *  - outputs returned through `T**` are host buffers owned by the caller until
 *    fgpu_free().
 *  - threading: ONE fgpu_ctx per process and device, shared by all host threads — the reference calls GraphBLAS
 *    from a worker pool on shared materialised handles (threadpool.rs:89-128, matrix.rs:781-796).  Every calling
 *    thread is bound, on its first call, to a LANE of the context: its own HIP stream, pinned staging block and
 *    free-list of device blocks, so concurrent calls never share a stream-ordered resource.  Any number of threads
 *    may concurrently call read-side entry points (fgpu_expand*, fgpu_mxm, fgpu_delta_lmxm, fgpu_mat_probe /
 *    extract / export, fgpu_vxm, fgpu_bfs, fgpu_pagerank, merges, transposes ...) on the SAME snapshots: a snapshot's
 *    stored content never changes, its acceleration indexes are built once under a per-snapshot mutex and
 *    published only when complete, and a call that returns a new fgpu_mat* synchronises its lane first whenever
 *    more than one lane exists, so a handle can be handed to another thread as soon as the call returns.
 *    What the caller keeps exclusive — exactly what the reference keeps exclusive (the caller's own F, a matrix
 *    under its `wait` mutex): an fgpu_bfs_plan is used by one thread at a time (run_async / wait on the same
 *    thread); fgpu_mat_free may be called from any thread once no call that takes the snapshot is executing
 *    (work other threads queued asynchronously is fenced inside the library); fgpu_set_option, fgpu_mat_build_tiles
 *    with explicit parameters and fgpu_prof_* are configuration / measurement calls made while no other call runs.
 *  - There is NO CPU fallback: without a HIP device fgpu_init fails with
 *    FGPU_DEVICE and nothing else can be called.
 */
#ifndef FGPU_H
#define FGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fgpu_ctx fgpu_ctx; /* one per process+device, shared by all threads (matrix::init, matrix.rs:116-185) */
typedef struct fgpu_mat fgpu_mat; /* immutable device CSR snapshot of one matrix layer        */
typedef struct fgpu_bfs_plan fgpu_bfs_plan; /* per-(A,At) BFS workspace + partition state       */

typedef int32_t fgpu_info;
#define FGPU_OK 0                  /* GrB_SUCCESS                */
#define FGPU_NO_VALUE 1            /* GrB_NO_VALUE               */
#define FGPU_NULL_POINTER (-2)     /* GrB_NULL_POINTER           */
#define FGPU_INVALID (-3)          /* GrB_INVALID_VALUE          */
#define FGPU_DIM_MISMATCH (-6)     /* GrB_DIMENSION_MISMATCH     */
#define FGPU_OOM (-102)            /* GrB_OUT_OF_MEMORY          */
#define FGPU_INSUFFICIENT_SPACE (-103) /* GrB_INSUFFICIENT_SPACE  */
#define FGPU_OUT_OF_BOUNDS (-105)  /* GrB_INDEX_OUT_OF_BOUNDS    */
#define FGPU_DEVICE (-7002)        /* GxB_GPU_ERROR              */

/* ---- lifecycle ---------------------------------------------------------- */

/* Replaces matrix::init -> GxB_init(GrB_NONBLOCKING, allocators) (matrix.rs:116-185).
 * `mal`/`fre` (nullable) are the host allocator hooks used for every buffer
 * handed back to the caller (the reference passes Redis' allocator). */
fgpu_info fgpu_init(fgpu_ctx** ctx, int device, void* (*mal)(size_t), void (*fre)(void*));
/* Replaces matrix::shutdown -> GrB_finalize (matrix.rs:214-221). */
fgpu_info fgpu_finalize(fgpu_ctx* ctx);
const char* fgpu_last_error(void);
void fgpu_free(fgpu_ctx* ctx, void* p);
/* Result arrays (`T**` outputs) of 256 KiB and more are PINNED host blocks from a pool the context keeps (SURVEY.md
 * §8b: "outputs are pinned-host buffers owned by the caller until fgpu_free"): the device fills them with one DMA, ids
 * widened to 64 bits by a kernel, and fgpu_free returns them to the pool (the first result of a size pays the pinning,
 * ~0.1 ms per MiB; later ones do not).  Smaller outputs come from `mal`.  fgpu_host_alloc hands the caller a block of
 * the same pool for the arrays the CALLER provides (level[] / parent[] of fgpu_bfs and fgpu_bfs_fetch, centrality[] of
 * fgpu_pagerank): entry points that write into caller memory check whether it is pinned (a pool block, or memory the
 * caller registered with HIP) and then DMA straight into it; pageable memory goes through a ring of four 2 MiB pinned
 * chunks and a host copy.  Release with fgpu_free.  (The reference's GrB_Vector results live in GraphBLAS-owned memory
 * and are read element by element, algo_procedures.rs:1096-1160; a maintainer's binding would allocate its level
 * vector here.) */
fgpu_info fgpu_host_alloc(fgpu_ctx* ctx, uint64_t bytes, void** out);
/* Run all subsequent work of the CALLING THREAD's lane on an externally owned hipStream_t
 * (plumbing for torch.distributed: pass torch.cuda.current_stream().cuda_stream).
 * NULL restores the lane's own stream. */
fgpu_info fgpu_set_stream(fgpu_ctx* ctx, void* hip_stream);
/* Wait for the work the calling thread has queued on its lane. */
fgpu_info fgpu_sync(fgpu_ctx* ctx);
/* Engine options (the analogue of GrB_Global_set_INT32, matrix.rs:151-159).  One name per line: accepted values, meaning;
 * "A/B" marks a switch kept for measurements, whose two sides give identical results.  A value outside what a line accepts,
 * and an unknown name, return FGPU_INVALID and leave the stored value as it was.  The defaults, and the measurements behind
 * them, are on the fields of fgpu_options (falkordb_amd/csrc/options.hpp).  Every option below except "transpose_wb" can be
 * read back with fgpu_get_option.
 *   LDS-tiled / blocked vxm
 *   "tiled_u"                   1, 2, 4, 8          items in flight per wavefront of the tiled kernel
 *   "tiled_nt"                  0 / not 0           nontemporal entry loads
 *   "tiled_threads"             256, 512, 1024      its workgroup size
 *   "tiled_wgs"                 0 .. 65536          its grid, 0 = one workgroup per CU
 *   "tiled_layout"              0 .. 2              full-pass pull layout: 0 = by size, 1 = tiled (x tile in LDS), 2 = blocked (output window in LDS too)
 *   "blocked_variant"           0 .. 3              kernel variant of the blocked layout (trips in flight / workgroups per CU)
 *   fgpu_expand* (k-hop chains)
 *   "expand_mode"               0 .. 2              0 = pick per hop, 1 = sorted-CSR products only, 2 = bit-parallel from the first hop
 *   "expand_bits_ratio"         1 .. 1024           expand_mode 0: a hop goes to bit form when its traversed edges exceed nnz / ratio
 *   "expand_row_groups"         0 / not 0           sparse mid-chain pull: 1 = a wavefront per 32-row group, 0 = a wavefront per row item
 *   "expand_records"            0 / not 0           sparse mid-chain pull: rows of at most 4 bits are read as records of source indices (A/B)
 *   "expand_group_items"        0, 1                ... its rows of at most 256 entries: 1 = a wavefront per item of the packed stream (fgpu_mat_group_items), 0 = a wavefront per 32-row group (A/B)
 *   "expand_fuse_count"         0 / not 0           fgpu_expand_count: 1 = the last bit-parallel hop counts its rows where it produces them, 0 = a separate pass counts
 *   "expand_compact"            0 / not 0           empty source rows are dropped before the chain goes to bits when that halves the row width (A/B)
 *   "expand_first_hop"          0 / not 0           a clean first hop from one-entry rows copies the source rows (A/B)
 *   "expand_emit_sort"          0 .. 2              bit state -> rows: 0 = ballot transpose, 2 = (row, vertex) pairs + stable sort by row, 1 = pairs + sort unless the result holds more than 8 entries per vertex
 *   "expand_xcd"                0 / not 0           dense count hop: 1 = rows of X gathered by the XCD that owns their partition, partial rows folded per vertex (A/B)
 *   "expand_xcd_relabel"        0 / not 0           ... the state it reads is laid out hot-first per partition (A/B)
 *   "expand_xcd_min_mb"         0 .. 1048576        ... taken when the bit state holds at least this many MiB
 *   "expand_nt"                 0 .. 7              ... streaming hints, a mask: 1 = partial rows stored non-temporal, 2 = column ids read non-temporal, 4 = the fold reads non-temporal
 *   "expand_xp_direct"          0, 1                ... 1 = a single-entry run is read from X by the fold, 0 = every run is streamed (A/B)
 *   "expand_xp_fold"            0, 1                ... the fold: 1 = index work once per row, one load per piece that exists, 0 = a slot per row and step loads all 8 partitions' rows (A/B)
 *   "expand_xp_fold_min_words"  2, 4, 8, 16, 32     ... the piece fold runs on bit rows of at least this many 64-bit words (32: none), narrower rows keep the slot fold
 *   "expand_xp_dense"           0, 1                ... the fold's groups: 1 = 64 consecutive ranks among the rows that have an in-edge, 0 = 64 consecutive vertex ids (A/B)
 *   "expand_xp_cut"             0, 1                ... the chunk table a new plan gets: 1 = chunks of whole double trips, 0 = the key cut (fgpu_mat_xp_chunks)
 *   "expand_xp_lookahead"       0, 1                ... 1 = the stream kernel carries its look-ahead into the wavefront's next chunk (A/B)
 *   "expand_xp_stream_wgs"      0 .. 65536          ... at most this many workgroups of the stream kernel per partition, 0 = as many as the chunks and the CUs allow
 *   "expand_scan_min"           0 .. 2^31 - 1       fgpu_expand_count: a call with more source rows than this is a whole-frontier call, cut into passes (0 = never)
 *   "expand_scan_rows"          64 .. 4096, 2^k     ... live rows per pass
 *   "expand_scan_lanes"         1 .. 16             ... lanes the passes are dealt to
 *   fgpu_bfs
 *   "bfs_wgs_per_cu"            1 .. 64             grid of the fused BFS level kernel, workgroups per CU
 *   "bfs_tiny"                  0 .. 2              consecutive tiny levels in one single-workgroup launch: 0 off, 1 on, 2 = when the plan's previous search took more than 12 levels
 *   "bfs_hub_first"             0 / not 0           pull levels read a copy of At whose rows are reordered by descending out-degree class
 *   "bfs_alive_rule"            0 / not 0           push <-> pull rule: 1 = the unvisited share over the vertices that have an in-edge, 0 = over all vertices
 *   "bfs_pb"                    0 .. 2              heavy push levels by propagation blocking: 0 off, 1 = plans of at least 2^24 vertices, 2 = every single-rank plan
 *   "bfs_pb_min_edges"          1 .. 2^63 - 1       ... a push level with at least this many edges goes that way
 *   "bfs_prof_split"            0 / not 0           a profiled plan launches the push / pull twins of the level kernel, told apart by name
 *   merges, transposes, results
 *   "merge_mode"                0 .. 2              fgpu_mat_merge: 0 = entry-parallel, 1 = a wavefront per row (pattern layers only), 2 = entry-parallel, every base entry of a touched row searching the deltas
 *   "merge_items"               0 / not 0           merge scatter: 1 = shifted copy by 2048-entry items, 0 = per word / per entry (A/B)
 *   "transpose_mode"            0 .. 3              pattern transpose / COO build: 0 = counting sort, 1 = COO rebuild through the sorter, 2 = LDS-staged levels, 3 = two levels
 *   "transpose_wb"              any                 low-digit bits of the counting transpose, 0 = pick; PROCESS-wide experiment knob, unchecked, not readable
 *   "pinned_results"            0 / not 0           result arrays from 256 KiB up come from the context's pinned pool and are filled by DMA
 *   "pinned_pool_mb"            0 .. 1048576        pinned blocks kept for reuse after fgpu_free, MiB
 *   algorithms
 *   "pagerank_parts"            0 .. 2              PageRank SpMV over 8 column ranges, one per XCD: 0 off, 1 = when the score vector exceeds one L2, 2 = always
 *   "wcc_mode"                  0 .. 2              fgpu_wcc: 0 = auto, 1 = Afforest with sampling and skip, 2 = one full link pass over every entry of A
 *   "bc_batch"                  0 .. 64             fgpu_betweenness: sources per batch, 0 = auto (16 / 32 / 64 by nsrc, halved to fit 3/4 of the free device memory)
 *   "bc_direction"              0 .. 2              fgpu_betweenness forward levels: 0 = auto by the entries each would read, 1 = push over A, 2 = pull over At
 *   "maxflow_global_every"      0 .. 1048576        fgpu_maxflow: pulses between two global relabels, 0 = the built-in period
 *   "sssp_delta_log2"           -1074 .. 1023, 4096 fgpu_sssp: the bucket width is 2^value, 4096 = derived from the graph
 *   "spdag_sides"               0 .. 3              fgpu_shortest_dag: which ball grows: 0 = the cheaper frontier, 1 = forward only, 2 = backward only, 3 = alternating
 *   multi-GPU BFS (fgpu_bfs_dist_run)
 *   "dist_collective"           0, 1                frontier exchange: 0 = grouped ncclSend / ncclRecv, 1 = one ncclBroadcast per rank
 *   "dist_timing"               0 / not 0           HIP events around every level kernel and exchange for fgpu_bfs_dist_times (~20 us of stream idle time per level)
 *   "dist_force_self"           0 / not 0           TEST ONLY: a communicator of ONE rank still issues the self send / recv, broadcast and all-reduce of a multi-rank exchange
 *   "dist_test_delay_us"        0 .. 100000         TEST ONLY: a kernel spinning this many microseconds behind every level kernel of this context's rank */
fgpu_info fgpu_set_option(fgpu_ctx* ctx, const char* name, int64_t value);
/* Reads the current value of any option fgpu_set_option stores (all of the list above but "transpose_wb"; 0 / not 0 options
 * read as 0 or 1), so a caller can put back what it found, or one of the measurement counters the context keeps.  The
 * counters have no setter; unknown names return FGPU_INVALID.
 *   "expand_kernel_launches"    kernels launched by fgpu_expand* on this context so far (the count of a batch is a difference of two reads)
 *   "expand_scan_last_live"     live source rows of the last whole-frontier fgpu_expand_count
 *   "expand_scan_last_passes"   ... and its passes
 *   "expand_xp_piece_folds"     launches of the piece fold of the XCD-partitioned count hop so far (which fold a call ran, and that the hop ran at all, is a difference of two reads)
 *   "expand_xp_slot_folds"      ... and of the slot fold
 *   "expand_xp_last_direct"     entries of A' the last partitioned count hop read straight from X as single-entry runs, 0 when its plan streams every run
 *   "expand_xp_last_groups"     groups its fold looped over: ceil(rows with an in-edge / 64), or ceil(rows / 64)
 *   "expand_xp_last_chunks"     chunks of the stream in its plan
 *   "expand_xp_last_shared_rows" ... and those that begin inside a run
 *   "expand_group_item_launches" launches of the sparse mid-chain pull in its packed-item form so far (expand_group_items)
 *   "bfs_pb_last_levels"        levels the search fgpu_bfs_stats last read ran by propagation blocking
 *   "bfs_cp_last_mask"          bit k: fused launch k of that search ran behind the list kernel (a sparse frontier listed into the queue, or a pull of listed candidates)
 *   "dist_self_calls"           forced self collectives issued so far (dist_force_self; tests/test_gpu_dist.py)
 *   "harmonic_last_entries"     the last fgpu_harmonic call: entries of the recomputed rows
 *   "harmonic_last_gathered"    ... and sketches gathered
 *   "sssp_last_delta_log2"      the last fgpu_sssp call: log2 of the bucket width it used, 1024 = one bucket for all
 *   "msf_last_entries_round<k>" the last fgpu_msf call: entries read in round k = 0 .. 31, the rounds past 31 in 31 */
fgpu_info fgpu_get_option(fgpu_ctx* ctx, const char* name, int64_t* value);
/* name[256]; returns CU count, wave size, LDS bytes per block, total HBM bytes. */
fgpu_info fgpu_device_info(fgpu_ctx* ctx, char* name, int32_t* cus, int32_t* wave,
                           int64_t* lds_bytes, int64_t* hbm_bytes);
/* Bytes currently held by the ctx's device pool (GRAPH.MEMORY analogue, graph.rs:3935). */
fgpu_info fgpu_device_bytes(fgpu_ctx* ctx, uint64_t* in_use, uint64_t* pooled);

/* ---- matrices ----------------------------------------------------------- */

/* Empty nrows x ncols matrix: Matrix::<bool>::new (matrix.rs:1214-1235). */
fgpu_info fgpu_mat_new(fgpu_ctx* ctx, fgpu_mat** out, uint64_t nrows, uint64_t ncols);

/* COO -> CSR with duplicate coordinates collapsed.
 * vals == NULL : Matrix::<bool>::build -> GxB_Matrix_build_Scalar (matrix.rs:1281-1303;
 *                dup-collapse pinned by matrix.rs:1686-1695).
 * vals != NULL : Matrix::<u64>::build -> GrB_Matrix_build_UINT64(..., GxB_ANY_UINT64)
 *                (matrix.rs:1186-1210); the LAST duplicate wins (a legal ANY). */
fgpu_info fgpu_mat_from_coo(fgpu_ctx* ctx, fgpu_mat** out, uint64_t nrows, uint64_t ncols,
                            const uint64_t* rows, const uint64_t* cols, const uint64_t* vals,
                            uint64_t n);

/* The inline value of a pair that holds several edges (MULTI_EDGE, tensor.rs:207). */
#define FGPU_MULTI_EDGE (~0ull)

/* One relationship type's bulk batch -> the three things a Tensor holds for it (tensor.rs:184-205, 333-455 run on an empty
 * tensor and folded; the batch shape of Graph::create_relationships_bulk + flush_for_bulk, graph.rs:2062-2140):
 *   fwd   UINT64 nrows x ncols, one entry per DISTINCT (src, dst): the edge id when the batch holds one edge of the pair,
 *         FGPU_MULTI_EDGE when it holds several;
 *   bwd   BOOL ncols x nrows, the transposed pattern;
 *   the multi-edge rows: multi_key[n_multi] ascending compound keys (src << 32 | dst), multi_off[n_multi + 1], and
 *         multi_ids[multi_off[n_multi]] with every run's ids ASCENDING whatever the input order.
 * Host arrays in; the arrays out are engine-owned (fgpu_free; multi_key and multi_ids are NULL when n_multi == 0, multi_off
 * always has its n_multi + 1 entries), the matrices the caller's until fgpu_mat_free.  n == 0 gives two empty matrices and
 * n_multi == 0.  Unlike fgpu_mat_from_coo with values ("the last duplicate wins") no id of a repeated pair is lost.
 * FGPU_INVALID, with fgpu_last_error set and nothing allocated, for: a coordinate at or past its dimension; a dimension past
 * the 32-bit id space (2^32 - 1 or more); n >= 2^32 - 1; an id equal to FGPU_MULTI_EDGE; the same (src, dst, id) triple
 * twice (edge ids are unique in the reference; the edge-by-edge path would leave a MULTI_EDGE pair with a one-id list).  The
 * context stays usable after an error.
 * stats (nullable): [0] distinct pairs, [1] multi-edge pairs, [2] ids in multi-edge runs, [3] longest run, [4] runs that
 * arrived out of ascending order — 0 for freshly allocated ascending ids — [5] of those, sorted on the device (up to 64 ids
 * in a wavefront, up to 4096 in a workgroup), [6] of those, longer than 4096 ids and sorted by the host after the read-back,
 * [7] sort path taken: 0 one workgroup (n < 4096), 1 the stable counting sort, 2 the same sort in 16-bit digits (a dimension
 * past 2^31). */
fgpu_info fgpu_edges_build(fgpu_ctx* ctx, uint64_t nrows, uint64_t ncols, const uint64_t* srcs, const uint64_t* dsts,
                           const uint64_t* ids, uint64_t n, fgpu_mat** fwd, fgpu_mat** bwd, uint64_t** multi_key,
                           uint64_t** multi_off, uint64_t** multi_ids, uint64_t* n_multi, uint64_t stats[8]);

/* DETACH DELETE of a node set on one matrix (Graph::delete_nodes + delete_implicit_edges, graph.rs:1698-1772, 2386-2494): the
 * entries incident to the nodes leave the matrix and its transposed pattern, and come back as the removal list.
 *   m      a BOOL or UINT64 snapshot; mt (nullable) the BOOL transposed pattern of m, what a Tensor holds as `mt`;
 *   nodes  a host array of n_nodes ids, any order, duplicates allowed; D is its set;
 *   sides  bit 0: the entries whose ROW is in D are dropped; bit 1: the entries whose COLUMN is in D are dropped.  1 serves the
 *          node x label matrix, 3 tensors and the adjacency.
 * m_out is m without the dropped entries: the same type, dimensions and values, sorted unique rows, stored hypersparse exactly
 * when fgpu_mat_from_coo would store that many populated rows of that dimension so.  mt_out is the same for mt with rows and
 * columns swapped; it must be non-NULL exactly when mt is.  Both are NEW snapshots (fgpu_mat_free): m and mt are untouched, and
 * whoever still reads them keeps reading them.
 * The removal list is wanted when rem_row is non-NULL (then rem_col, rem_val, n_rem and n_rem_out must be too) and needs mt:
 *   the first n_rem_out triples (rem_row, rem_col, rem_val)[k] = (s, d, v) are the OUT entries, those with s in D under bit 0, in
 *   ascending (s, d) — a self-loop on a node of D appears here only;
 *   the other n_rem - n_rem_out are the IN entries, those with d in D under bit 1 that are not out entries (s not in D when bit
 *   0 is set), in ascending (d, s): the order in which a walk of mt's rows meets them.
 * v is the value m stores — for a tensor the inline edge id or FGPU_MULTI_EDGE — and 0 for a BOOL m.  The arrays are
 * engine-owned (fgpu_free) and NULL when n_rem == 0.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated and the context still usable, for: a node id at or past a dimension
 * it indexes (the rows under bit 0, the columns under bit 1); sides outside 1..3; a list wanted with bit 1 on a matrix that is
 * not square; mt of other dimensions than ncols x nrows, or valued; a list wanted without mt.  n_nodes == 0 gives copies of the
 * inputs and an empty list.
 * stats (nullable): [0] distinct nodes in D, [1] out entries and [2] in entries of the list (0 when none is wanted), [3] removed
 * entries of m whose value is FGPU_MULTI_EDGE, [4] entries kept in m_out, [5] entries kept in mt_out; [6], [7] are 0.
 * Work: one lane per stored entry of m and of mt, every output placed by a scan. */
fgpu_info fgpu_nodes_detach(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* nodes, uint64_t n_nodes,
                            int sides, fgpu_mat** m_out, fgpu_mat** mt_out, uint64_t** rem_row, uint64_t** rem_col,
                            uint64_t** rem_val, uint64_t* n_rem, uint64_t* n_rem_out, uint64_t stats[8]);

/* DELETE r of a batch of edges on one relationship type (Graph::delete_relationships over Tensor::remove_all, graph.rs:2268-2373,
 * tensor.rs:454-629): n triples (srcs, dsts, ids)[k] leave the tensor's matrices.
 *   m      the tensor's folded UINT64 base: a value is an inline edge id or FGPU_MULTI_EDGE; mt its BOOL transposed pattern;
 *   multi_key / multi_off / multi_ids  the multi-edge rows of the pairs the caller believes the batch touches, in the shape
 *          fgpu_edges_build returns them: n_multi keys src << 32 | dst strictly ascending, multi_off[0] = 0, every run at least 2
 *          ids long and strictly ascending.  A key that is not a FGPU_MULTI_EDGE entry of m is ignored.
 * The slow path of tensor.rs:497-629 restated as set operations (it applies a removal only where the id is there, so the order
 * of the batch does not matter): a triple HITS when (src, dst) is stored in m and either its inline value equals id, or the value
 * is FGPU_MULTI_EDGE and id is in the pair's supplied row.  hit[k] (the caller's n bytes, nullable) = 1 for every hitting triple,
 * each duplicate of one included; multi_taken[j] (the caller's multi_off[n_multi] bytes, required when n_multi > 0) = 1 iff some
 * triple hit multi_ids[j].  A single-edge pair that is hit leaves m and mt.  A multi-edge pair with 2 or more ids left keeps
 * FGPU_MULTI_EDGE; with 1 left it is demoted: m_out stores the surviving id inline; with 0 left it leaves m and mt.  An unknown
 * id, an id of another pair and an absent pair change nothing.  This is the reference's result whenever every triple names a
 * stored edge, which Graph::delete_relationships guarantees by resolving the ids first.  On an unknown id the reference's
 * no-multi fast path (tensor.rs:467-495) drops the pair whatever the id; this call deliberately does not.
 * m_out / mt_out are NEW snapshots (fgpu_mat_free) with sorted unique rows, stored hypersparse exactly when fgpu_mat_from_coo
 * would store that many populated rows of that dimension so; m and mt are untouched.  emp_row / emp_col [n_emp] are the pairs
 * that left m, ascending in (src, dst): engine-owned (fgpu_free), NULL when n_emp == 0.  n == 0 gives copies of the inputs.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated and the context still usable, for: a coordinate at or past its
 * dimension; n >= 2^32 - 1; an id equal to FGPU_MULTI_EDGE; m not valued; mt missing, valued or of other dimensions than
 * ncols x nrows; keys not strictly ascending, a run shorter than 2, ids not ascending in a run; a triple whose pair holds
 * FGPU_MULTI_EDGE in m with no row supplied for it (counted on the device and read back with the totals).
 * stats (nullable): [0] triples that hit, [1] pairs emptied, [2] of those, pairs that were multi-edge, [3] pairs demoted,
 * [4] entries kept in m_out, [5] entries kept in mt_out, [6] triples whose pair is absent, [7] triples whose pair is stored but
 * whose id is unknown.
 * Work: a lane per triple (binary searches), a lane per supplied row, a lane per stored entry of m and of mt; every output is
 * placed by a scan. */
fgpu_info fgpu_edges_remove(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* srcs, const uint64_t* dsts,
                            const uint64_t* ids, uint64_t n, const uint64_t* multi_key, const uint64_t* multi_off,
                            const uint64_t* multi_ids, uint64_t n_multi, fgpu_mat** m_out, fgpu_mat** mt_out, uint8_t* hit,
                            uint8_t* multi_taken, uint64_t** emp_row, uint64_t** emp_col, uint64_t* n_emp, uint64_t stats[8]);

/* CREATE of a built batch onto a relationship type that already holds edges (Tensor::set_all_from_slices under
 * Graph::create_relationships_bulk, tensor.rs:333-447, graph.rs:2062-2121): the union of a loaded tensor with one batch, both in
 * the shape fgpu_edges_build returns.
 *   m / mt      the tensor's folded UINT64 base (a value is an inline edge id or FGPU_MULTI_EDGE) and its BOOL transposed pattern;
 *   fwd / bwd   the same two matrices of the batch, of m's and mt's dimensions;
 *   a_key / a_off / a_ids [n_a]  the multi-edge rows of the pairs of m the caller believes the batch touches;
 *   b_key / b_off / b_ids [n_b]  the rows fgpu_edges_build returned with fwd.
 * Row arrays follow fgpu_edges_remove's rules: keys src << 32 | dst strictly ascending, off[0] = 0, every run at least 2 ids long
 * and strictly ascending.  An a key that is not a FGPU_MULTI_EDGE entry of m, or that names a pair the batch does not, is
 * ignored; so is a b key that is not a FGPU_MULTI_EDGE entry of fwd.
 * The per-edge transitions of tensor.rs:383-418 restated per pair of fwd: a pair absent from m enters m_out with fwd's value;
 * a pair stored in both COLLIDES — m_out holds FGPU_MULTI_EDGE and the pair's id list is the ascending merge of m's side (the
 * inline id, or the a row under FGPU_MULTI_EDGE) with fwd's side (the inline id, or the b row).  Pairs of m the batch does not
 * name keep their value.  mt_out is the pattern union of mt and bwd.
 * o_key / o_off / o_ids hold one row per colliding pair, keys and ids ascending, every row at least 2 ids long; the rows of
 * multi-edge pairs only the batch names are the caller's b rows and are not copied back.  The arrays are engine-owned
 * (fgpu_free); o_key and o_ids are NULL when n_o == 0, o_off always has n_o + 1 entries.
 * m_out / mt_out are NEW snapshots (fgpu_mat_free) with sorted unique rows, stored hypersparse exactly when fgpu_mat_from_coo
 * would store that many populated rows of that dimension so; the four input matrices are untouched.  An empty fwd gives copies of
 * m and mt and n_o = 0.  The call keeps no device memory.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated and the context still usable, for: m or fwd not valued; mt or bwd
 * missing, valued or of other dimensions than ncols x nrows; fwd of other dimensions than m; keys not strictly ascending, a run
 * shorter than 2, ids not ascending in a run, an id equal to FGPU_MULTI_EDGE in a row; a colliding pair that holds
 * FGPU_MULTI_EDGE in m with no a row, or in fwd with no b row; an id on BOTH sides of a colliding pair (the edge is already
 * stored: edge ids are unique, the same stance as fgpu_edges_build's "same triple twice") — the last three counted on the
 * device and read back before any output is allocated; row ids and entries of fwd that could merge into 2^32 - 1 ids or more.
 * stats (nullable): [0] pairs new to m, [1] colliding pairs (= n_o), [2] of those, pairs that held an inline id in m (promoted),
 * [3] of those, pairs that held FGPU_MULTI_EDGE in m (extended), [4] ids in the out rows, [5] longest out row, [6] entries of
 * m_out, [7] entries of mt_out.
 * Work: a lane per stored entry of fwd and of bwd (binary searches), a lane per output id (a co-rank search over the two
 * sides), a lane per stored entry of m and of mt; every output is placed by a scan. */
fgpu_info fgpu_edges_union(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* a_key, const uint64_t* a_off,
                           const uint64_t* a_ids, uint64_t n_a, const fgpu_mat* fwd, const fgpu_mat* bwd, const uint64_t* b_key,
                           const uint64_t* b_off, const uint64_t* b_ids, uint64_t n_b, fgpu_mat** m_out, fgpu_mat** mt_out,
                           uint64_t** o_key, uint64_t** o_off, uint64_t** o_ids, uint64_t* n_o, uint64_t stats[8]);

/* Host CSR (what GxB_unload_Matrix_into_Container yields: p, i, x [, h];
 * matrix.rs:508-546) -> device snapshot.  rowptr has nvec+1 entries when
 * `hyper_rows` (sorted non-empty row ids, nvec of them) is given, else
 * nrows+1.  rowptr_bits / colidx_bits are 32 or 64.  Rows must already be
 * sorted and unique (the state after Matrix::wait). */
fgpu_info fgpu_mat_from_csr(fgpu_ctx* ctx, fgpu_mat** out, uint64_t nrows, uint64_t ncols,
                            uint64_t nnz, const void* rowptr, int rowptr_bits,
                            const void* colidx, int colidx_bits, const uint64_t* vals,
                            const uint64_t* hyper_rows, uint64_t nvec);

/* Synthetic Graph500 R-MAT adjacency generated ON DEVICE (bench/tests data):
 * 2^scale vertices, edge_factor*2^scale raw edges, (a,b,c) quadrant probabilities
 * as 16.16 fixed point (0 -> Graph500 defaults .57/.19/.19), counter-based
 * splitmix64 keyed by `seed`, vertex ids scrambled by a fixed bijection, directed,
 * self-loops dropped, duplicates collapsed.  Not a reference API. */
fgpu_info fgpu_mat_rmat(fgpu_ctx* ctx, fgpu_mat** out, int scale, int edge_factor,
                        uint64_t seed, uint32_t a16, uint32_t b16, uint32_t c16);

fgpu_info fgpu_mat_free(fgpu_mat* m);                       /* Drop, matrix.rs:387-399 */
fgpu_info fgpu_mat_nrows(const fgpu_mat* m, uint64_t* out);  /* GrB_Matrix_nrows */
fgpu_info fgpu_mat_ncols(const fgpu_mat* m, uint64_t* out);  /* GrB_Matrix_ncols */
fgpu_info fgpu_mat_nvals(const fgpu_mat* m, uint64_t* out);  /* GrB_Matrix_nvals, matrix.rs:722-729 */
fgpu_info fgpu_mat_has_values(const fgpu_mat* m, int32_t* out);

/* D2H export of the whole snapshot in CSR form (GxB_Container p/i/x):
 * rowptr[nrows+1] (always full, hyper rows expanded), colidx[nnz], vals[nnz] or NULL. */
fgpu_info fgpu_mat_export_csr(fgpu_ctx* ctx, const fgpu_mat* m, uint64_t** rowptr,
                              uint64_t** colidx, uint64_t** vals, uint64_t* nnz);
/* Entries of rows [min_row, max_row] in ascending (row, col) order:
 * matrix::Iter::new/next (matrix.rs:1471-1605). */
fgpu_info fgpu_mat_extract(fgpu_ctx* ctx, const fgpu_mat* m, uint64_t min_row, uint64_t max_row,
                           uint64_t** rows, uint64_t** cols, uint64_t** vals, uint64_t* n);

/* GrB_transpose full: Matrix::transpose (matrix.rs:633-662).  Pattern only when
 * `a` is BOOL; values carried when UINT64. */
fgpu_info fgpu_mat_transpose(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a);

/* Batched point probes (K11): GrB_Matrix_extractElement_* / GxB_Matrix_isStoredElement
 * (matrix.rs:731-737, 1158-1172, 1248-1262).  present[i] = 1 iff (rows[i], cols[i])
 * is stored; vals (nullable) receives the u64 value (0 for BOOL). */
fgpu_info fgpu_mat_probe(fgpu_ctx* ctx, const fgpu_mat* m, const uint64_t* rows,
                         const uint64_t* cols, uint64_t n, uint8_t* present, uint64_t* vals);

/* Delta merge (K3/K6): out = (m \ dm) U dp, dp's value wins on a shared coordinate
 * (GrB_SECOND_UINT64) — VersionedMatrix::flush / extract (versioned_matrix.rs:609-620,
 * 892-938), Tensor::flush (tensor.rs:702-751).  dp/dm may be NULL.
 * `dm_masks_dp`: 0 => dp entries survive dm (extract / Tensor structure semantics,
 * where the invariants make it moot), 1 => eWiseAdd<!dm>(m, dp) exactly as flush's
 * (true,true) arm (mask applies to the whole union). */
fgpu_info fgpu_mat_merge(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* m, const fgpu_mat* dp,
                         const fgpu_mat* dm, int dm_masks_dp);
/* The same merge with the values dropped: out = pattern((m \ dm) U dp), a BOOL snapshot in one pass —
 * Tensor::extract (tensor.rs:838-850), Matrix::set_pattern = GrB_Matrix_apply(GxB_ONE_BOOL)
 * (matrix.rs:906-924), and with dp = dm = NULL the plain structure copy of a UINT64 layer that
 * build_relationship_matrix_unrestricted / build_adjacency_matrix start from (graph.rs:2520-2549, 3870-3894). */
fgpu_info fgpu_mat_merge_pattern(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* m, const fgpu_mat* dp,
                                 const fgpu_mat* dm, int dm_masks_dp);
/* GrB_Matrix_resize (Matrix::resize, matrix.rs:576-598; the `grown` re-emit of tensor.rs:613-667):
 * a new snapshot of `a` at nrows x ncols; every entry keeps its coordinate and value, entries at or
 * past the new dims are dropped (grown fixture: matrix.rs:1617-1672). */
fgpu_info fgpu_mat_resize(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a, uint64_t nrows,
                          uint64_t ncols);
/* Pattern intersection (K7): eWiseMult ANY_PAIR (matrix.rs:876-896); values from `b`. */
fgpu_info fgpu_mat_intersect(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a, const fgpu_mat* b);
/* intersection_nvals (matrix.rs:743-761). */
fgpu_info fgpu_mat_intersect_nvals(fgpu_ctx* ctx, const fgpu_mat* a, const fgpu_mat* b,
                                   uint64_t* out);

/* Acceleration index for the dense-frontier vxm (tiled.hip): regroup the entries of `m` by column
 * tile of 2^tile_bits ids so the kernel can stage the frontier tile in LDS and stream packed 4-byte
 * entries from HBM.  tile_bits / vec / k == 0 pick defaults (2^20-id tiles = 128 KiB of LDS).
 * Logically const: the matrix content is unchanged; the index is owned and freed by the matrix.
 * No reference counterpart (GraphBLAS keeps its own internal formats, matrix.rs:405-426). */
fgpu_info fgpu_mat_build_tiles(fgpu_ctx* ctx, fgpu_mat* m, int tile_bits, int vec, int k);
/* info[0]=tile_bits [1]=tiles [2]=64-row groups [3]=items [4]=padded entries [5]=vec [6]=k
 * [7]=device bytes of the index.  FGPU_NO_VALUE when the matrix has no tiles. */
fgpu_info fgpu_mat_tiles_info(const fgpu_mat* m, uint64_t info[8]);
/* The packed item stream the sparse mid-chain pull of fgpu_expand* reads the rows of at most 256 entries of m's cached
 * transpose from (built here if no hop has built it yet): item i is hdr[4 i ..] = (first row, rows 1 .. 32, entries <= 256, 0)
 * and the 256 words cols[256 i ..], each a column id in bits 0..26 under its row-in-item in bits 27..31, the tail 0xFFFFFFFF.
 * Items hold whole consecutive rows, cut greedily in row order; rows of more than 256 entries count as empty.  Both arrays are
 * released with fgpu_free.  FGPU_NO_VALUE when the matrix is empty or the stream does not apply (2^27 - 1 columns or more).
 * The option expand_group_items picks the form of the pull that runs, the counter expand_group_item_launches counts the packed one. */
fgpu_info fgpu_mat_group_items(fgpu_ctx* ctx, const fgpu_mat* m, uint32_t** hdr, uint32_t** cols, uint64_t* nitems);
/* The chunk table of the XCD-partitioned count hop's plan on m's cached transpose (built here, under the options in force, if no
 * hop has built it yet), read back as 32-bit words: [chunks, cut, first entry of partition 0 .. 8, first chunk of partition 0 .. 8],
 * then for every chunk the first entry, then for every chunk the run (= partial row) of that entry, then for every chunk 1 when
 * that run began in an earlier chunk.  `cut` is the cut the plan holds: 1 = every chunk but a partition's last is a multiple of 128
 * entries, 0 = the key cut.  Released with fgpu_free.  FGPU_NO_VALUE when the matrix has no such plan.
 * The option expand_xp_cut picks the cut a new plan gets; the counters expand_xp_last_chunks and expand_xp_last_shared_rows
 * describe the plan of the last count hop. */
fgpu_info fgpu_mat_xp_chunks(fgpu_ctx* ctx, const fgpu_mat* m, uint32_t** words, uint64_t* nwords);

/* ---- products (ANY_PAIR structural semiring) ------------------------------ */

/* C = F x B, no mask: Matrix::lmxm -> GrB_mxm(GxB_ANY_PAIR_BOOL) (matrix.rs:930-947).
 * The result is a new snapshot (the reference overwrites F in place; the caller
 * frees the old F). */
fgpu_info fgpu_mxm(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* b);

/* C = (F x (m U dp)) with every (i,j) of (F x dm) removed from the F x m part —
 * the exact algebra of Matrix::delta_lmxm (matrix.rs:1317-1402): dp results are
 * NOT masked; the mask is row-level (any source of row i tombstoning j kills
 * (i,j)).  dp / dm may be NULL or empty => plain lmxm. */
fgpu_info fgpu_delta_lmxm(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* m,
                          const fgpu_mat* dp, const fgpu_mat* dm);

/* The device core of CondTraverseOp::expand_batch (cond_traverse.rs:452-751):
 *   F[i, src_ids[i]] = 1 for i in [0,nsrc)  (src_ids[i] == UINT64_MAX => row i left empty:
 *   a source that failed its label pre-filter, cond_traverse.rs:561-589);
 *   F <- delta_lmxm(F; m[h], dp[h], dm[h]) for h in [0,nhops);
 *   entries whose dest lacks a bit in `dst_label_bitmap` (nullable, ncols bits,
 *   LSB-first in 64-bit words) are dropped (cond_traverse.rs:644-651);
 *   output CSR over the nsrc rows, dest ascending & unique per row
 *   (= the ascending (row_i, dest) stream of F.iter, cond_traverse.rs:644).
 * dp[h] / dm[h] may be NULL.  flops (nullable) receives sum over hops of
 * sum_{(i,s) in F_h} deg_{m U dp}(s) — the traversed-edge count used for TEPS. */
fgpu_info fgpu_expand(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                      const fgpu_mat* const* m, const fgpu_mat* const* dp,
                      const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                      uint64_t** out_rowptr, uint64_t** out_dest, uint64_t* out_nnz,
                      uint64_t* flops);

/* fgpu_expand with the result in the device's own 32-bit form: out_rowptr[nsrc + 1] and out_dest[nnz] are uint32_t (the
 * engine's row pointers and node ids are 32-bit throughout; a result of 2^32 entries or more is refused by every emitting
 * entry) — two DMAs of the arrays as they lie, nothing widened on the device or the host, half the PCIe bytes of fgpu_expand.
 * Release both with fgpu_free. */
fgpu_info fgpu_expand32(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                      const fgpu_mat* const* m, const fgpu_mat* const* dp,
                      const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                      uint32_t** out_rowptr, uint32_t** out_dest, uint64_t* out_nnz,
                      uint64_t* flops);

/* Same chain, the result F left on the device as a matrix handle — what the reference holds between
 * `F = delta_lmxm(...)` and `F.iter(...)` (cond_traverse.rs:602-608: F IS a Matrix<bool>; its rows are then walked
 * with the row iterator, :644).  *out is a BOOL snapshot with nsrc rows (row i = source i), dest ascending and unique
 * per row, already filtered by `dst_label_bitmap`; read it with fgpu_mat_extract / fgpu_mat_export_csr, release it with
 * fgpu_mat_free.  fgpu_expand = this + one export of the whole result into host arrays. */
fgpu_info fgpu_expand_mat(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                          const fgpu_mat* const* m, const fgpu_mat* const* dp,
                          const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                          fgpu_mat** out, uint64_t* flops);

/* The same chain with the result as the two COLUMNS CondTraverseOp::expand_batch hands on (cond_traverse.rs:644-751: walk
 * (row_i, dest) ascending; drop a destination that differs from a pre-bound `to`, :657-661; emit `gather(out_indices)` +
 * NodeIds): out_row[q] = index of the source row of pair q (uint16_t or uint32_t per `row_bits`; a child batch holds at most
 * 1024 rows, batch.rs:81), out_dest[q] = its destination, pairs ascending by (row, dest).  `pinned_dest` (nullable, nsrc
 * entries): ~0 = the row keeps every destination, anything else = the row keeps only that destination if it is reached.  Both
 * columns are built on the device (row indices expanded from the row pointers, the pinned rows cut down by a binary search)
 * and arrive by DMA in pinned blocks of the context's pool — the host never walks the result.  Release both with fgpu_free;
 * *out_n = 0 leaves both NULL. */
fgpu_info fgpu_expand_pairs(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                            const fgpu_mat* const* m, const fgpu_mat* const* dp,
                            const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                            const uint64_t* pinned_dest, int row_bits, void** out_row, uint64_t** out_dest,
                            uint64_t* out_n, uint64_t* flops);

/* The same two columns with the destinations as the 32-bit node ids the device holds (node ids of a traversed graph fit 32
 * bits: Tensor's multi-edge keys demand it, tensor.rs:154-163): half the bytes over PCIe for the column that IS the result —
 * without pinned rows it is the chain's own column-id array, copied out as it lies — and what CondTraverseOp's C++ twin takes
 * (falkordb_amd/host/graph.cpp: ExpandedRows widens on access, where the reference's NodeId(u64) is needed).  Otherwise
 * identical to fgpu_expand_pairs. */
fgpu_info fgpu_expand_pairs32(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                            const fgpu_mat* const* m, const fgpu_mat* const* dp,
                            const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                            const uint64_t* pinned_dest, int row_bits, void** out_row, uint32_t** out_dest,
                            uint64_t* out_n, uint64_t* flops);

/* The same chain when EVERY row has a pre-bound destination — CondTraverse with `to` bound on the whole batch, the multi-hop
 * ExpandInto shape `MATCH (a)-[*]->(b) ... MATCH (a)-->()-->(b)` (tests/flow/test_expand_into.py:63-95; the reference runs
 * the whole chain and drops every destination but the bound one, cond_traverse.rs:657-661): present[i] = 1 iff dst_ids[i]
 * is reached from src_ids[i] by the chain (and passes the destination label).  The hops before the last run as in
 * fgpu_expand; the last one is ONE entry of (F·m)<not (F·dm)> U (F·dp) per row — in bit form one bit of one row of the
 * state, found by walking the in-neighbours of dst_ids[i]; in sorted-CSR form a binary search per frontier entry — so no
 * result is materialised, emitted or copied back.  present[nsrc] is a HOST array; *flops (nullable) counts the traversed
 * edges of the hops that ran (the last hop is not expanded). */
fgpu_info fgpu_expand_probe(fgpu_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, uint64_t nsrc,
                            const fgpu_mat* const* m, const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                            const uint64_t* dst_label_bitmap, uint8_t* present, uint64_t* flops);

/* The same chain as a PATTERN PREDICATE — `WHERE (p)-[:KNOWS]->()`, `WHERE NOT ...`, the right branch of SemiApply /
 * AntiSemiApply / OrApplyMultiplexer with an unbound destination (semi_apply.rs:85-106; the reference runs the branch over
 * the batch, emits every match and keeps the set of origin rows).  Contract: bit i of match_bits is set iff row i of
 * fgpu_expand over the same arguments is non-empty.  The conventions are fgpu_expand's and fgpu_expand_probe's:
 * src_ids[i] == UINT64_MAX leaves row i empty, dp / dm are nullable as arrays and per hop, hypersparse layers are taken, the
 * errors are fgpu_expand's.  The hops before the last run as in fgpu_expand; the last hop is NOT expanded: a row matches as
 * soon as one frontier vertex has a label-passing dp entry, or a label-passing m entry whose column no entry of the last dm
 * names (no tombstone can mask it for any row).  The last hop's rule is the row-level mask (F·m)<not (F·dm)> U (F·dp), so the
 * rows that reach only columns named by dm are undecided: they run the whole chain once more, those rows alone.
 *   match_bits   HOST array of (nsrc + 63) / 64 words, bit i & 63 of word i >> 6; the padding bits past nsrc are 0.
 *   flops        nullable: the traversed edges of the hops that ran (hops 0 .. nhops - 2 of the call; not the exact pass).
 *   stats        nullable: [0] rows matched, [1] undecided rows sent through the exact pass, [2] adjacency entries the last
 *                step read (all layers), [3] the form that answered: 0 a sorted-CSR frontier, 1 the bit state.
 * nsrc == 0 is a no-op. */
fgpu_info fgpu_expand_exists(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                             const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                             const uint64_t* dst_label_bitmap, uint64_t* match_bits, uint64_t* flops, uint64_t stats[4]);

/* One tensor's multi-edge rows (`me`, tensor.rs:184-205) resident on the device, in the shape fgpu_edges_build returns them and
 * fgpu_edges_remove checks them: n_multi keys src << 32 | dst strictly ascending, off[0] = 0, every run at least 2 ids long and
 * strictly ascending, no id equal to FGPU_MULTI_EDGE.  Host arrays in (copied); n_multi == 0 gives an empty table.  A malformed
 * table returns FGPU_INVALID with nothing kept.  fgpu_multi_size: rows and ids held (either pointer nullable). */
typedef struct fgpu_multi fgpu_multi;
fgpu_info fgpu_multi_new(fgpu_ctx* ctx, const uint64_t* key, const uint64_t* off, const uint64_t* ids, uint64_t n_multi,
                         fgpu_multi** out);
fgpu_info fgpu_multi_free(fgpu_multi* t);
fgpu_info fgpu_multi_size(const fgpu_multi* t, uint64_t* n_multi, uint64_t* n_ids);

/* The per-row path of CondTraverse (CondTraverseOp::expand_row + process_pairs, cond_traverse.rs:758-1117, without the
 * attribute filters, the sibling-edge filter and the cross-row dedup) for a whole batch of k rows over n_types relationship
 * tensors given in SCAN order (edge_type_indices, :418-426 — the order of the pattern's names, not ascending ids).
 *   from / to [k]   a node id, or ~0 for unbound.  A row with both unbound is skipped (the full-matrix walk stays host code).
 *   m / dp / dm     per type the forward layers: m UINT64 (inline edge id or FGPU_MULTI_EDGE), dp UINT64 and dm (pattern) nullable —
 *                   the array itself or any element; all square and of one dimension n < 2^32 - 1.
 *   mt_m / mt_dp / mt_dm   per type the BOOL layers of the transposed structure (Tensor::matrix_t); mt_m is required exactly when
 *                   some pass of some row walks incoming entries (its matrix destination is bound and its source is not).
 *   multi           per type the tensor's fgpu_multi, nullable when it holds no FGPU_MULTI_EDGE.
 *   flags           FGPU_EDGES_TRANSPOSED: the pattern runs against the storage direction (`from` is the matrix destination);
 *                   FGPU_EDGES_BIDIRECTIONAL: a second pass with the endpoints swapped, self-loops dropped there;
 *                   FGPU_EDGES_FIRST_ONLY: one representative id per pair, as !emit_relationship (:1063-1081).
 *   from_bitmap / to_bitmap   nullable (n + 63) / 64-word node sets, applied to the ORIENTED from_node / to_node of every pair.
 *                   build_state (:376-389) hands process_pairs the labels of the matrix source and destination per pass:
 *                   (from, to) forward and (to, from) in reverse, swapped again under `transposed`; process_pairs orients the
 *                   pair by the same rule (from_node = the matrix destination on a reverse walk), so in both passes and under
 *                   `transposed` the four lists reduce to: from_node carries the source labels, to_node the destination labels.
 * Per row: the forward pass has matrix source = transposed ? to : from and the other endpoint as matrix destination.  A bound
 * source walks that row of the effective structure (pattern(m) \ dm) U pattern(dp) by ascending column, cut to the destination
 * when that is bound too; with only the destination bound, that row of the transposed structure by ascending source.  The
 * bidirectional pass follows the row's forward pass.  The pair set is the union over the types; per pair, in that order, the
 * types are scanned in the given order and each emits the ids of Tensor::get(mat_src, mat_dst) ascending: dp's value wins over
 * m's, a dm entry hides m's, FGPU_MULTI_EDGE expands to the table's row.  FIRST_ONLY keeps the first id of each (row, pass, pair).
 * Out: out_row / out_from / out_to (uint32_t) and out_id (uint64_t), *out_n entries each, row ascending and then as above;
 * duplicate rows of the batch each get their own output rows.  out_pass (nullable: not wanted) receives a fifth column, 0 for an id
 * of the forward pass and 1 for the reverse pass — what tells the pair (a, b) walked forward from the pair (b, a) walked in
 * reverse, which orient to the same (from_node, to_node).  Engine-owned blocks (pinned from 256 KiB up, filled by DMA),
 * released with fgpu_free; NULL when *out_n == 0.  k == 0 or n_types == 0 gives *out_n = 0.  The call keeps no device memory.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated and the context still usable, for: a bound id at or past n; layers
 * that are not all n x n; an unvalued m (or dp); a missing mt_m where one is needed; k above 2^24, n_types above 64, unknown flag
 * bits; walked entries or emitted ids that reach 2^32 - 1; a visited pair that holds FGPU_MULTI_EDGE with no table row (counted
 * on the device and read back before any output is allocated, as fgpu_edges_remove does).
 * stats (nullable): [0] stored entries walked outgoing, [1] stored entries walked incoming, [2] ids emitted, [3] multi-edge
 * pairs expanded, [4] longest emitted list of one (pair, type), [5] the ordering path: 0 = the entry positions gave the order (one
 * type, no dp layer), 1 = one stable sort on (row, pass, other node), 2 = two stable sorts (other node, then (row, pass)),
 * [6] (pair, type) items that emitted, [7] row segments (row x pass x type x layer) of the batch.
 * Work: a lane per segment (binary searches), a lane per walked entry (value resolved by binary search), a lane per emitted id;
 * every output is placed by a scan; no wavefront-per-row loop. */
#define FGPU_EDGES_TRANSPOSED 1
#define FGPU_EDGES_BIDIRECTIONAL 2
#define FGPU_EDGES_FIRST_ONLY 4
fgpu_info fgpu_expand_edges(fgpu_ctx* ctx, const uint64_t* from, const uint64_t* to, uint64_t k, const fgpu_mat* const* m,
                            const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                            const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                            int n_types, int flags, const uint64_t* from_bitmap, const uint64_t* to_bitmap, uint32_t** out_row,
                            uint32_t** out_from, uint32_t** out_to, uint64_t** out_id, uint8_t** out_pass, uint64_t* out_n,
                            uint64_t stats[8]);

/* indegree(n [, types]) / outdegree(n [, types]) (entity.rs:268-381, runtime.rs:1727-1796, graph.rs:1839-1887) for a batch of k
 * nodes, or for every node, in one call: per position and direction the number of (src, dst, id) triples that
 * Tensor::iter(id, id, transposed) yields, summed over the n_types tensors in the given order — a type given twice counts
 * twice (graph.rs:1856-1860).
 *   nodes [k]       node ids, each below the dimension n; a repeated id gets its own answer per position; k <= 2^24.
 *                   NULL is the WHOLE-GRAPH form: k must equal n, position i is node i, and any n the layers allow is taken.
 *   m .. multi      the tensors' layers and tables exactly as fgpu_expand_edges takes them (0 to 64 types; dp / dm / mt_* / multi
 *                   nullable as array or element).  The transposed layers are read only under FGPU_DEGREE_IN, and a missing
 *                   mt_m[t] is then FGPU_INVALID.
 *   flags           FGPU_DEGREE_OUT, FGPU_DEGREE_IN or both; 0 and any other bit are FGPU_INVALID.
 *   out_degree / in_degree   HOST arrays of k words, required with the matching flag and not touched without it.
 * Value: over the effective structure (pattern(m) \ dm) U pattern(dp) of the node's row (outgoing), or of its row in the
 * transposed layers (incoming), 1 per pair whose Tensor::eff_get value is an inline id and the length of the table row per pair
 * that holds FGPU_MULTI_EDGE; a pair in both dp and m counts once, with dp's value; a self-loop counts once in each direction.
 * On every input fgpu_expand_edges accepts this is the number of rows it emits for from = node (outgoing), or for to = node
 * under the storage direction (incoming), with no flag and no bitmap.  The incoming half of that equality assumes mt_* hold
 * the transposed structure of the forward layers, as a Tensor keeps them: a (type, incoming) answered from the row pointers of
 * mt_m never looks at the forward dp / dm, where fgpu_expand_edges reads the forward value of every incoming entry.
 * Both forms walk their positions in windows of at most "degree_window_rows" rows (an engine option read and set through
 * fgpu_get_option / fgpu_set_option: 64 .. 2^24, default 2^24; it is kept beside the option table), fewer when rows x
 * directions x types x layers of a window would reach 2^31 segments.
 * FGPU_INVALID, with fgpu_last_error set and the context still usable, for: an id at or past n (before anything is written);
 * k above 2^24 in the batch form, k != n in the whole-graph form; layers that are not all n x n, an unvalued m (or dp);
 * n_types above 64; a window whose walked entries reach 2^32 - 1 (lower degree_window_rows); a pair read as FGPU_MULTI_EDGE
 * whose table has no row (counted on the device and read back before the window's results are copied out; the windows before it
 * of a whole-graph call have been written).  n_types == 0 or k == 0 gives zeros and FGPU_OK.
 * stats (nullable, all 0 after a failure): [0] (position, type, direction) triples answered by the row-pointer tier, [1] stored
 * entries walked outgoing, [2] stored entries walked incoming, [3] multi-edge pairs met, [4] longest id list met, [5] the sum
 * of the out-degrees, [6] the sum of the in-degrees, [7] windows walked.
 * Work: a (type, direction) whose walked side has no dp, no dm and no table (multi[t] NULL or empty: fgpu_multi's contract lets
 * that be only when the tensor holds no FGPU_MULTI_EDGE) is the row-pointer tier: a lane per (position, type, direction) adds
 * the row's length and reads no entry.  Every other one is the entry tier, fgpu_expand_edges' segments and gather without its
 * sort, placement and columns: a lane per segment, one scan, a lane per walked entry that applies the shadow and tombstone
 * searches and resolves 1 or the list length, then the wavefront's counts are summed by position with shuffles and added with
 * one 64-bit atomic per (wavefront, position, direction).  Integer sums commute: the result does not depend on scheduling.
 * The outputs are k words per direction; the call keeps no device memory. */
#define FGPU_DEGREE_OUT 1
#define FGPU_DEGREE_IN 2
fgpu_info fgpu_node_degrees(fgpu_ctx* ctx, const uint64_t* nodes, uint64_t k, const fgpu_mat* const* m,
                            const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                            const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                            int n_types, int flags, uint64_t* out_degree, uint64_t* in_degree, uint64_t stats[8]);

/* CondVarLenTraverse, the [*min..max] operator (cond_var_len_traverse.rs:81-387, VarLenIter), for a whole batch of k rows in one
 * call, without the attribute / WHERE filters.  start [k]: the bound endpoint of every row; dest (nullable array): a node id the
 * other endpoint must equal, or ~0 for unbound.  m .. multi, n_types: the relationship tensors in the pattern's order, as for
 * fgpu_expand_edges.  dst_label_bitmap: nullable (n + 63) / 64-word node set the emitted endpoint must lie in.
 *   Direction   no flag: the walk follows outgoing edges; FGPU_TRAILS_REVERSED: incoming edges; FGPU_TRAILS_BIDIRECTIONAL: both.
 *               The two together are FGPU_INVALID (the reference never builds that combination, :534).
 *   Adjacency   of a node v (get_node_relationships_by_type, graph.rs:1797-1835): the types in the given order — a type listed
 *               twice is walked twice — and per type first the outgoing half, by ascending (dst, id) over the effective structure
 *               (m \ dm) U dp, the ids those of Tensor::get (dp's value wins, FGPU_MULTI_EDGE expands to the table row, ascending),
 *               then, when incoming edges are walked, the incoming half by ascending (src, id) over the transposed layers, the
 *               self-loop left out of it only when the outgoing half was walked too.  This is type-major, not the pair-major order
 *               of fgpu_expand_edges.
 *   Trails      a frame is (node, used edge ids, depth); the root is (start, {}, 0).  A candidate whose edge id is already on
 *               the frame's trail is dropped — by id only, across types and directions (:247).  A child at hop = depth + 1 emits
 *               when hop >= min_hops, its node equals the row's dest if one is bound, and its node passes the bitmap; it goes on
 *               as a frame when hop < max_hops (UINT32_MAX = unbounded).  The 0-hop row (start, start) comes first when
 *               min_hops == 0 and the start passes the dest and bitmap tests, with n_types == 0 too.
 *   Order       rows ascending; within a row exactly the reference's: frames are visited in DFS preorder with the children
 *               visited last-first (the LIFO stack), and a visited frame contributes its emitting children in adjacency order,
 *               all before any deeper frame does (:379-383).  Duplicate rows of the batch each get their own output.
 *   Out         out_row / out_from / out_to / out_hops (uint32_t), *out_n entries: (from, to) oriented to the pattern — (start,
 *               other), or (other, start) under REVERSED; out_hops the trail's length.  With FGPU_TRAILS_PATHS emission i has
 *               out_path_off[i + 1] - out_path_off[i] edges at out_path_edge[out_path_off[i] ..] and one more node at
 *               out_path_node[out_path_off[i] + i ..], both in pattern order, that is reversed under REVERSED (path_value,
 *               :134-147); without the flag the three path pointers must be NULL.  Engine-owned blocks (pinned from 256 KiB up,
 *               filled by DMA), released with fgpu_free; all NULL when *out_n == 0.  The call keeps no device memory.
 *   Budget      trails grow exponentially, so the caller sets max_items: the frames (the k roots included) plus the emissions the
 *               call may hold.  Past it the call returns FGPU_INSUFFICIENT_SPACE with nothing allocated for output and stats
 *               holding what was counted up to that point; exactly at the budget is FGPU_OK.  The same code when a trail would go
 *               on as a frame deeper than FGPU_TRAILS_MAX_DEPTH edges (frames at that depth are still expanded, so max_hops up to
 *               FGPU_TRAILS_MAX_DEPTH + 1 always fits, and an unbounded pattern fits when no trail outgrows the depth), or when
 *               one level walks 2^32 - 1 entries or more.  The level's counts are read back before its buffers are allocated.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated and the context still usable, for: a start or bound dest at or past
 * n; non-square or mismatched layers; an unvalued m (or dp); a missing mt_m when incoming entries are walked; k above 2^24, n_types
 * above 64, unknown flag bits or REVERSED with BIDIRECTIONAL; path pointers without PATHS; a walked pair that holds
 * FGPU_MULTI_EDGE without a table row; max_items == 0 or at or past 2^32 - 1.
 * stats (nullable): [0] frames expanded, [1] adjacency entries walked, [2] candidates dropped as already used, [3] emissions,
 * [4] levels run, [5] how the level step orders a node's entries: 0 = the entry positions are the adjacency order (no dp layer in
 * any type), 1 = the m and dp runs of every (frame, type, half) are merged by rank (a binary search per entry; no sort is needed
 * for two sorted runs), [6] multi-edge pairs expanded, [7] peak items held (frames + emissions).
 * Work: level-synchronous — a lane per (frame, type, half, layer) segment, a lane per walked entry, a lane per candidate id, every
 * frame and emission placed by a scan; the order is two scans per level more. */
#define FGPU_TRAILS_REVERSED 1
#define FGPU_TRAILS_BIDIRECTIONAL 2
#define FGPU_TRAILS_PATHS 4
#define FGPU_TRAILS_MAX_DEPTH 64
fgpu_info fgpu_expand_trails(fgpu_ctx* ctx, const uint64_t* start, const uint64_t* dest, uint64_t k, const fgpu_mat* const* m,
                             const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                             const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                             int n_types, int flags, uint32_t min_hops, uint32_t max_hops, const uint64_t* dst_label_bitmap,
                             uint64_t max_items, uint32_t** out_row, uint32_t** out_from, uint32_t** out_to, uint32_t** out_hops,
                             uint64_t** out_path_off, uint32_t** out_path_node, uint64_t** out_path_edge, uint64_t* out_n,
                             uint64_t stats[8]);

/* The weighted pair matrix algo.MSF (algo_procedures.rs:1403-1704), algo.SPpaths (:2156-2257, :2405-2514) and the hop-bounded
 * pruning table start from, built from the tensors' own layers in one call: per ordered node pair the smallest weight over the
 * selected relationship types, their multi-edges and the traversal direction, and the relationship that was kept.
 *   m / dp / dm / multi   the forward layers and multi-edge tables of n_types tensors, as for fgpu_expand_edges and under the same
 *                   rules: all n x n with n = m[0]'s dimension < 2^32 - 1, m and dp valued, dp / dm / multi nullable (the array or
 *                   any element), 1 to 64 types.  No transposed layer is needed.  A type given twice (the same four handles)
 *                   changes nothing, the stats included.
 *   Examined        per type the effective relationships of Tensor::iter_edges: every pair of (pattern(m) \ dm) U pattern(dp), dp's
 *                   value winning over m's, FGPU_MULTI_EDGE expanding to the table's row.  Self-loops are not examined at all,
 *                   neither is a relationship with an end outside active_bitmap (nullable, (n + 63) / 64 words): they are not
 *                   counted and not refused.
 *   Weight          attr_ids [n_attr] strictly ascending (checked on the device), attr_vals [n_attr].  A relationship weighs
 *                   attr_vals[k] where attr_ids[k] equals its id (binary search); an id that is not listed - below the first,
 *                   above the last or in a gap - weighs `missing`.  Then, in this order: FGPU_PAIRS_NEGATE negates a LISTED value
 *                   (`missing` is not negated); -0.0 becomes +0.0; FGPU_PAIRS_DROP_NONFINITE leaves NaN and +-inf relationships
 *                   out; FGPU_PAIRS_REFUSE_NEGATIVE fails the call on a finite weight < 0.  attr_ids == NULL: every relationship
 *                   weighs 1.0, `missing` and NEGATE are ignored.
 *   Direction       FGPU_PAIRS_OUT: a relationship (src, dst) is a candidate of the ordered pair (src, dst); FGPU_PAIRS_IN: of
 *                   (dst, src); both: of both, and the result is symmetric.
 *   Kept            per ordered pair the candidate with the smallest (key(weight), id), key the order of fgpu_msf: IEEE totalOrder
 *                   of the binary64 bit pattern with -0.0 = +0.0.  A NaN that was not dropped is ordered by its bits.  The kept
 *                   candidate is a function of the candidate set only; no floating-point atomic takes part.
 *   Out             *W: n x n UINT64 of binary64 bit patterns - a BOOL pattern when attr_ids == NULL; *K: the same pattern, UINT64,
 *                   the kept relationship id (with attr_ids == NULL the smallest id of the pair).  Ordinary snapshots with sorted
 *                   columns, freed with fgpu_mat_free, usable by fgpu_msf / fgpu_sssp / fgpu_sssp_hops / fgpu_mat_probe as they
 *                   are.  W == NULL or K == NULL: that matrix is not wanted.  Nothing examined gives empty n x n matrices.  The call
 *                   keeps no device memory on its inputs.
 * FGPU_INVALID, with fgpu_last_error set, nothing allocated, *W and *K untouched and the context still usable, for: n_types outside
 * 1 .. 64 (with no type there is no dimension); layers that are not all n x n; an unvalued m (or dp); unknown flag bits, or neither
 * OUT nor IN; attr_ids not strictly ascending; stored entries, relationships or candidates that reach 2^32 - 1; an examined pair
 * that holds FGPU_MULTI_EDGE with no table row (counted on the device and read back before any output is allocated, as
 * fgpu_expand_edges does); a refused weight - *refused_id (nullable) is then the smallest refused relationship id and
 * fgpu_last_error reads "fgpu_pair_weights: relationship <id> has a negative weight".
 * stats (nullable; all 0 after a failure): [0] stored entries examined (live pairs of a type), [1] relationships examined (after
 * multi-edge expansion), [2] candidates (after the drop and the direction), [3] pairs out, [4] relationships dropped as non-finite,
 * [5] relationships that took `missing`, [6] multi-edge pairs expanded, [7] most candidates of one pair.
 * Work: a lane per stored entry of every m and dp (the dm / dp checks by binary search), a lane per relationship (the ids of a
 * multi-edge row placed by a scan, the attribute by binary search), candidates placed by a scan and grouped per pair by the stable
 * counting sorts of fgpu_edges_build, a lane per sorted position closing the runs and taking the run's minimum through integer
 * atomicMin, row pointers off a scan; no wavefront-per-row loop. */
#define FGPU_PAIRS_OUT 1
#define FGPU_PAIRS_IN 2
#define FGPU_PAIRS_NEGATE 4
#define FGPU_PAIRS_DROP_NONFINITE 8
#define FGPU_PAIRS_REFUSE_NEGATIVE 16
fgpu_info fgpu_pair_weights(fgpu_ctx* ctx, const fgpu_mat* const* m, const fgpu_mat* const* dp, const fgpu_mat* const* dm,
                            const fgpu_multi* const* multi, int n_types, int flags, const uint64_t* active_bitmap,
                            const uint64_t* attr_ids, const double* attr_vals, uint64_t n_attr, double missing,
                            fgpu_mat** W, fgpu_mat** K, uint64_t* refused_id, uint64_t stats[8]);

/* The same chain with the result STREAMED to the host in chunks of whole source rows — the shape in which
 * CondTraverseOp::expand_batch consumes it (cond_traverse.rs:644-751: walk (row_i, dest) ascending, emit an output batch
 * every 1024 pairs): the chain runs once, F stays on the device, and chunks of at most `chunk_rows` consecutive source
 * rows are copied into a ring of four pinned buffers, three copies on the link while the caller walks the fourth.
 *   open : runs the chain; *nnz / *flops (nullable) as fgpu_expand.  dest_bits = 64 (GrB_Index ids, widened on the device)
 *          or 32 (half the bytes on the link; node ids fit 32 bits, tensor.rs:154-163).
 *   next : blocks until the next chunk has landed; *first_row / *nrows name its source rows, rowptr[0 .. nrows] are entry
 *          offsets relative to the chunk (rowptr[0] = 0), dest[0 .. rowptr[nrows]) the destinations (uint64_t or
 *          uint32_t per dest_bits), ascending and unique per row.  The arrays stay valid until the next call on the
 *          stream.  Returns FGPU_NO_VALUE (and *nrows = 0) after the last chunk.
 *   close: releases the device result and the ring (valid at any point).
 * A stream belongs to the thread that opened it. */
typedef struct fgpu_expand_stream fgpu_expand_stream;
fgpu_info fgpu_expand_stream_open(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                                  const fgpu_mat* const* m, const fgpu_mat* const* dp,
                                  const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                                  uint64_t chunk_rows, int dest_bits, fgpu_expand_stream** out,
                                  uint64_t* nnz, uint64_t* flops);
fgpu_info fgpu_expand_stream_next(fgpu_expand_stream* s, uint64_t* first_row, uint64_t* nrows,
                                  const uint64_t** rowptr, const void** dest);
fgpu_info fgpu_expand_stream_close(fgpu_expand_stream* s);

/* Same as fgpu_expand but the result stays on device and only its size and an
 * order-independent checksum come back (full-size configs whose output would not
 * fit a host buffer): checksum = sum over the (row, dest) entries of
 * mix64(row) * (mix64(dest ^ 0x9e3779b97f4a7c15) | 1) mod 2^64, mix64 = the splitmix64 finaliser (a product of a row
 * hash and a destination hash: the bit-parallel state sums it per vertex through look-up tables instead of per entry).
 * A call with more source rows than the whole-frontier bound (see fgpu_set_option) is cut into passes of live rows.  All
 * three sums are linear in the rows, so over a hop 0 without delta entries the sources whose ONLY out-edge in m[0] ends at
 * the same vertex are counted as one row: the row carries the sum of their row hashes, and its nnz and flops are multiplied
 * by the number of sources it stands for.  The results are those of the row-by-row count, bit for bit; the passes counter
 * reports the passes that ran, the live counter the live source rows. */
fgpu_info fgpu_expand_count(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                            const fgpu_mat* const* m, const fgpu_mat* const* dp,
                            const fgpu_mat* const* dm, int nhops,
                            const uint64_t* dst_label_bitmap, uint64_t* out_nnz,
                            uint64_t* checksum, uint64_t* flops);

/* Variable-length reachability core (BASELINE config 5).  The reference evaluates
 * `[*1..k]` with a per-row DFS (CondVarLenTraverseOp, cond_var_len_traverse.rs:81-128); its DISTINCT
 * end-point set and the per-hop frontiers are set algebra over the same layers: ONE chain of `nhops` hops
 * (each hop a delta_lmxm, quirk included) evaluated once in bit form (one bit per source row),
 *   hop_nnz[h] / hop_checksum[h] : size / checksum of F x A_1 .. A_{h+1}  (walks of exactly h+1 hops),
 *   union_nnz / union_checksum   : the DISTINCT (row, dest) pairs reached by 1..nhops hops
 *                                  (= MATCH (a)-[*1..k]->(b) RETURN DISTINCT a, b; also the pruning set for the DFS).
 * hop_checksum / union_* / flops are nullable; checksum as in fgpu_expand_count; the destination-label
 * bitmap (nullable) filters every reported set.  Base matrices must be non-hypersparse with nnz < 2^31. */
fgpu_info fgpu_expand_levels(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                             const fgpu_mat* const* m, const fgpu_mat* const* dp,
                             const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                             uint64_t* hop_nnz, uint64_t* hop_checksum, uint64_t* union_nnz,
                             uint64_t* union_checksum, uint64_t* flops);

/* Exact trail counts for variable-length patterns of at most two hops.  The reference's `[*1..k]`
 * DFS emits one row per TRAIL (edge-unique path, cond_var_len_traverse.rs:196-387); for exactly `nhops` (1 or 2) hops
 * the number of trails from source i to a destination is a counting product over the effective layers (m \ dm) U dp:
 * PLUS_PAIR on pattern layers, PLUS_TIMES on UINT64 layers holding per-pair edge multiplicities (`weighted`), less the
 * length-2 walks that cross one self-loop twice.  Output CSR over the nsrc rows: dest ascending, count > 0.  Longer
 * trails have no product form (a walk may revisit an edge): use fgpu_expand_levels' reachable sets to prune the DFS. */
fgpu_info fgpu_expand_trail_counts(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                                   const fgpu_mat* const* m, const fgpu_mat* const* dp,
                                   const fgpu_mat* const* dm, int nhops, int weighted,
                                   uint64_t** out_rowptr, uint64_t** out_dest, uint64_t** out_count,
                                   uint64_t* out_nnz);

/* ---- boolean vxm / BFS (K9) ---------------------------------------------- */

/* w<!mask, replace> = f x A over the boolean (ANY_PAIR) semiring, vectors as
 * ncols-/nrows-bit bitmaps (LSB-first 64-bit words, HOST pointers; copied in/out).
 * This is GrB_vxm (graphblas/mod.rs:11173) in the form LAGraph's BFS issues it.
 * mask may be NULL.  `At` (nullable) enables the pull direction; `direction`:
 * 0 = auto (push over A while fewer than 1 / 32 of the vertices are in the frontier, else — given At — the LDS-tiled
 * pull), 1 = push over A, 2 = pull over At's CSR (full pass, no early exit),
 * 3 = pull over At's LDS-tile layout (built on first use, fgpu_mat_build_tiles). */
fgpu_info fgpu_vxm(fgpu_ctx* ctx, uint64_t* w, const uint64_t* f, const uint64_t* mask,
                   const fgpu_mat* A, const fgpu_mat* At, int direction);

/* PageRank: replaces LAGr_PageRank(&centrality, &iters, G, damping, tol, itermax, msg) as called by
 * algo.pageRank (algo_procedures.rs:741-752 with 0.85 / 1e-4 / 100; binding lagraph_bindings.rs:549-558) on the
 * adjacency matrix A (At nullable: transposed internally).  FP32 like the reference's GrB_FP32 vectors; sinks
 * (vertices without out-edges) spread their score evenly.  `active_bitmap` (nullable, nrows bits) restricts the run
 * to the induced subgraph of the flagged vertices — the label-filtered form (algo_procedures.rs:725-733) — and
 * leaves 0 in the other slots.  centrality[nrows] is a HOST array; *iters (nullable) the iterations taken. */
fgpu_info fgpu_pagerank(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                        float damping, float tol, int32_t itermax, float* centrality, int32_t* iters);
/* The same run; *converged (nullable) = 1 when the last iteration changed the scores by no more than tol, 0 when itermax
 * ended it first — what LAGr_PageRank turns into LAGRAPH_CONVERGENCE_FAILURE (lagraph_bindings.rs:549-558). */
fgpu_info fgpu_pagerank_status(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                               float damping, float tol, int32_t itermax, float* centrality, int32_t* iters,
                               int32_t* converged);

/* Weakly connected components: replaces LAGr_ConnectedComponents(&component, G, msg) as called by algo.WCC
 * (algo_procedures.rs:789-880; binding lagraph_bindings.rs:521-526).  The graph is undirected: every stored entry (i, j) of
 * A joins i and j.  `At` (nullable) is A's transpose; NULL is the caller's promise that A's pattern is symmetric (LAGraph's
 * is_symmetric_structure) — the Afforest path skips the giant component's rows and needs both directions of every edge.
 * `active_bitmap` (nullable, nrows bits, as fgpu_pagerank) restricts the run to the induced subgraph of the flagged vertices;
 * the other slots get -1.  component[nrows] is a HOST array (filled by DMA when pinned — fgpu_host_alloc — by staging
 * otherwise): component[v] = the smallest vertex id of v's component, the labelling LAGraph's FastSV converges to.
 * stats (nullable): [0] components among the active vertices, [1] adjacency entries read by the link kernels, [2] link
 * launches, [3] size of the component the sampling phase picked as the giant (0 when it did not run).  Option "wcc_mode":
 * 0 auto, 1 Afforest with sampling and skip, 2 one full link pass over every entry of A.  nrows == 0 is a no-op. */
fgpu_info fgpu_wcc(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                   int64_t* component, uint64_t stats[4]);

/* Community detection by label propagation: replaces LAGraph_cdlp(&out, G, itermax, msg) as called by algo.labelPropagation
 * (algo_procedures.rs:1168-1270; binding lagraphx_bindings.rs:218-223).  Synchronous label propagation as LDBC Graphalytics
 * defines CDLP and as LAGraph computes it for an undirected graph (LAGraph's source is not vendored; these are the rules):
 *   - label_0[v] = v;
 *   - iteration t computes every label_t[v] from label_{t-1} only (two buffers);
 *   - label_t[v] = the label that occurs most often among the stored entries (v, w) of v's row, each entry voting once with
 *     label_{t-1}[w]; ties go to the smallest label;
 *   - a stored diagonal entry votes like any other entry; a vertex with no voting entry keeps its label;
 *   - the run stops after itermax iterations, or earlier after the first iteration that changes no label.  Running out of
 *     iterations is not an error: the usual period-2 oscillation on bipartite structure is part of the algorithm.
 * LAGraph numbers its initial labels from 1 (label_0[v] = v + 1): the partition is identical, because the tie-break order is
 * the same, and every label here is LAGraph's minus 1.
 * `S` is the symmetric pattern (A (+) A'); symmetry is the caller's promise, like At == NULL in fgpu_wcc, and there is no
 * (A, At) form.  The matrix is a boolean pattern: a (row, col) pair given twice to a builder is one entry and one vote.
 * `active_bitmap` (nullable, nrows bits, as fgpu_pagerank) selects the induced subgraph: entries whose column is inactive do
 * not vote, and the inactive slots of label[] get -1.  label[nrows] is a HOST array (filled by DMA when pinned —
 * fgpu_host_alloc — by staging otherwise).  stats (nullable): [0] iterations run, [1] vertices whose label changed in the last
 * iteration run (0 = converged), [2] adjacency entries read, summed over the iterations, [3] distinct labels among the active
 * vertices at the end.  Errors: NULL ctx / S / label: FGPU_NULL_POINTER; non-square S: FGPU_DIM_MISMATCH; itermax < 0:
 * FGPU_INVALID.  itermax == 0 returns the identity labelling; nrows == 0 is a no-op.  The output is deterministic. */
fgpu_info fgpu_cdlp(fgpu_ctx* ctx, const fgpu_mat* S, const uint64_t* active_bitmap, int32_t itermax, int64_t* label,
                    uint64_t stats[4]);

/* Harmonic centrality by HyperBall: replaces LAGr_HarmonicCentrality(&scores, &reachable, G, node_weights, msg) as called by
 * algo.HarmonicCentrality (algo_procedures.rs:2623-2784) with an iso boolean directed adjacency.  Every vertex carries a
 * HyperLogLog sketch of its out-ball; an iteration is a pull over the semiring (merge = bytewise max, second).  The sketch
 * operators are those of the reference's PreJIT kernels; LAGraph's driver and its hash are not vendored, these are the rules:
 *   - sketch: m = 1024 registers of uint8 (1 KiB per vertex); the monoid identity is all zeros, merge is the bytewise max;
 *   - hash: a vertex v is its row index in A (ids fit u32).  h = (u32)v; h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13;
 *     h *= 0xc2b2ae35; h ^= h >> 16 (mod 2^32: the murmur3 32-bit finaliser, a bijection).  slot = h >> 22; w = h & 0x3FFFFF;
 *     rank = 1 + the number of leading zeros of w written in 22 bits (1..22), 23 when w == 0.  Vertex 0: slot 0, rank 23;
 *   - count(C): S = sum 2^-C[i] (exact in FP64 in any order: dyadic terms >= 2^-23, sum <= 1024); E = amm / S with
 *     amm = 0.7213 / (1 + 1.079 / 1024) * 1024^2; if E <= 2560 and Z, the number of zero registers, is > 0:
 *     E = 1024 log(1024 / Z); else if E > 2^32 / 30: E = -2^32 log(1 - E / 2^32).  All FP64;
 *   - C_0[v] is zero except v's own (slot, rank); est_0[v] = count(C_0[v]); score[v] = 0;
 *   - iteration t = 1, 2, ...: C_t[v] = the bytewise max of C_{t-1}[v] and of C_{t-1}[w] over the stored entries (v, w) of
 *     row v, from C_{t-1} only (two buffers).  A boolean pattern: a duplicate entry is one entry, a diagonal entry is harmless.
 *     If C_t[v] differs bytewise from C_{t-1}[v]: score[v] += (count(C_t[v]) - est_{t-1}[v]) / t and est_t[v] = the new count;
 *     otherwise nothing changes for v, exactly;
 *   - the run ends after the first iteration that changes no sketch (it contributes nothing).  Registers only grow: at most
 *     diameter + 1 iterations, and no itermax, as in the LAGraph signature.
 * score[v] is FP64.  reachable[v] = llround(est_final[v]) - 1, the vertices v reaches NOT counting v itself — this engine's
 * decision (the reference's tests only order it).  A vertex with no out-entry has score exactly 0.0 and reachable 0.
 * `active_bitmap` (nullable, nrows bits, as fgpu_pagerank) selects the induced subgraph: inactive columns contribute nothing,
 * inactive slots get score 0.0, reachable -1 and a zero sketch; the hashes stay those of the original row indices.
 * Every merge order gives the same bytes, so the output is deterministic; an implementation may skip entries whose column
 * did not change in the previous iteration (HyperBall's "modified" rule) — the result is bit-identical.
 * score[nrows] and reachable[nrows] are HOST arrays (filled by DMA when pinned — fgpu_host_alloc — by staging otherwise);
 * registers (nullable) receives the final nrows x 1024 sketch bytes.  stats (nullable): [0] iterations that changed at least
 * one sketch, [1] sketch changes summed over the iterations, [2] the largest reachable, [3] vertices with a non-zero score.
 * Workspace: 2 nrows KiB plus a few vectors; an allocation that does not fit returns FGPU_OOM, nothing is truncated.
 * Errors: NULL ctx / A / score / reachable: FGPU_NULL_POINTER; non-square A: FGPU_DIM_MISMATCH; nrows >= 2^32 - 1:
 * FGPU_INVALID.  nrows == 0 is a no-op.  fgpu_get_option "harmonic_last_entries" / "harmonic_last_gathered": the entries of
 * the rows the last call recomputed and the sketches it gathered, summed over its iterations. */
fgpu_info fgpu_harmonic(fgpu_ctx* ctx, const fgpu_mat* A, const uint64_t* active_bitmap, double* score, int64_t* reachable,
                        uint8_t* registers, uint64_t stats[4]);

/* Minimum spanning forest (Boruvka): replaces LAGraph_msf(&forest_edges, &component_id, A, sanitize = false, msg) as called by
 * algo.MSF (algo_procedures.rs:1272-1857; binding lagraphx_bindings.rs:261-267) with a symmetric FP64 matrix over compact
 * node ids.  LAGraph's source is not vendored; these are the rules:
 *   - W is square and symmetric — pattern AND values — by the caller's promise (LAGraph's sanitize = false, like At == NULL in
 *     fgpu_wcc).  A valued snapshot holds one IEEE-754 binary64 BIT PATTERN per entry in its uint64 value; a BOOL snapshot
 *     means every weight is 1.0;
 *   - diagonal entries are ignored.  `active_bitmap` (nullable, nrows bits, as fgpu_pagerank) selects the induced subgraph:
 *     entries with an inactive end are ignored;
 *   - every unordered pair {v, w} is ONE edge with the key (K(bits), min(v, w), max(v, w)), compared lexicographically.  K
 *     replaces 0x8000000000000000 (-0.0) by 0, then flips all bits of a negative pattern and only the sign bit of a
 *     non-negative one: the IEEE totalOrder with -0.0 = +0.0.  +-inf are ordinary weights (the reference scores a missing
 *     attribute +inf); a NaN is not an error, it sorts beyond the infinity of its sign;
 *   - that order is strict and total, so the minimum spanning forest under it is UNIQUE: it is the result, whatever order the
 *     kernels race in, bit-identical from run to run.
 * component (nullable, HOST array of nrows, filled by DMA when pinned — fgpu_host_alloc): component[v] = the smallest vertex
 * id of v's tree, the labelling of fgpu_wcc; -1 for inactive vertices.  The forest comes back once per edge as (row < col),
 * sorted ascending by (row, col), in three engine-owned arrays released with fgpu_free (pinned from 256 KiB up, like the
 * arrays of fgpu_mat_export_csr; NULL when the forest is empty).  forest_weights[k] is the stored value of entry (row, col),
 * bit-exact (-0.0 stays -0.0), or 1.0 for a BOOL W.  *n_forest = the active vertices minus the components.
 * Broken promise: if W(v, w) and W(w, v) differ, or only one of them is stored, WHICH forest comes back is unspecified, but the
 * call still returns FGPU_OK and the result is still a forest of (active - components) edges whose ends share a component: an
 * edge is recorded only by the hook that actually joined two trees, never because a component merely chose it.
 * stats (nullable): [0] Boruvka rounds, [1] forest edges, [2] adjacency entries read, summed over the rounds (rows whose
 * entries were all internal in an earlier round are not read again), [3] components among the active vertices.
 * Errors: NULL ctx / W / any of the four forest outputs: FGPU_NULL_POINTER; non-square W: FGPU_DIM_MISMATCH; nrows >= 2^32 - 1:
 * FGPU_INVALID; an allocation that does not fit: FGPU_OOM.  nrows == 0 is a no-op with *n_forest = 0.  fgpu_get_option
 * "msf_last_entries_round<k>", k = 0..31: the entries the last call read in round k (the round that found nothing included; the
 * rounds past 31 are added into 31). */
fgpu_info fgpu_msf(fgpu_ctx* ctx, const fgpu_mat* W, const uint64_t* active_bitmap, int64_t* component,
                   uint64_t** forest_rows, uint64_t** forest_cols, double** forest_weights, uint64_t* n_forest,
                   uint64_t stats[4]);

/* Maximum flow (synchronous push-relabel): replaces LAGr_MaxFlow(&f, &flow_mtx, NULL, G, src, sink, msg) as called by
 * algo.maxFlow (algo_procedures.rs:2786-3248, the call at 3112-3216) with an FP64 capacity matrix over compact node ids.
 * LAGraph's source is not vendored; these are the rules:
 *   - C is square; C(u, v) is the capacity of the arc u -> v.  A valued snapshot holds one IEEE-754 binary64 BIT PATTERN per
 *     entry in its uint64 value; a BOOL snapshot means every capacity is 1.0.  A hypersparse C is accepted;
 *   - a diagonal entry, and an entry whose capacity is <= 0 (-0.0 included), carries no flow and is ignored;
 *   - a NaN or infinite capacity anywhere in C is FGPU_INVALID: inf - inf must never reach a residual;
 *   - there is no active bitmap: the caller compacts the node ids, as the reference does.
 * *max_flow = the value of a maximum src -> sink flow.  The three engine-owned arrays (released with fgpu_free, pinned from
 * 256 KiB up like fgpu_msf's forest arrays; NULL when empty) hold one entry per arc of C that carries flow > 0, sorted
 * ascending by (row, col).  What comes back is a FLOW, not a preflow:
 *   - 0 < f(u, v) <= C(u, v) for every returned entry;
 *   - inflow = outflow at every vertex other than src and sink;
 *   - the net outflow of src = the net inflow of sink = *max_flow;
 *   - where both C(u, v) and C(v, u) exist, at most one of the two carries flow.
 * The VALUE is unique.  The ASSIGNMENT is not: which maximum flow comes back depends on the order the kernels' atomics land
 * in and may differ from run to run; every one of them satisfies the rules above.
 * Arithmetic is FP64 throughout, sums and differences of capacities only.  Every operation is EXACT when all capacities are
 * integers, or dyadic rationals with a common exponent, and their sum stays below 2^53 (in units of that exponent): then the
 * rules above hold with equality, bit for bit.  Otherwise they hold to the rounding of the sums (conservation to a few ulps
 * of the largest capacity per arc of the vertex).
 * No path from src to sink: 0.0 and *n_flow = 0.
 * stats (nullable): [0] push / relabel pulses that had an active vertex, [1] global relabels, [2] arcs of the residual network
 * (two per unordered pair of vertices joined by a live arc), [3] pushes.
 * Errors: NULL ctx / C / max_flow / n_flow / any of the three flow outputs: FGPU_NULL_POINTER; non-square C:
 * FGPU_DIM_MISMATCH; src or sink >= nrows, src == sink, nrows >= 2^32 - 1, nnz >= 2^31 - 2^24 (the residual
 * network holds up to 2 nnz entries at 32-bit positions): FGPU_INVALID.  The pulse loop has
 * a hard cap of 4 (n^2 + n) pulses — beyond the relabel bound of the algorithm, never reached by a correct run — past which
 * the call returns FGPU_INVALID with a message instead of running on.  fgpu_set_option "maxflow_global_every": pulses between
 * two global relabels (0 = the built-in choice). */
fgpu_info fgpu_maxflow(fgpu_ctx* ctx, const fgpu_mat* C, uint64_t src, uint64_t sink, double* max_flow,
                       uint64_t** flow_rows, uint64_t** flow_cols, double** flow_vals, uint64_t* n_flow,
                       uint64_t stats[4]);

/* Single-source shortest paths over non-negative FP64 weights (near / far delta-stepping): the numeric core of algo.SPpaths'
 * single-path branch (run_path_algo -> dijkstra_single_path, algo_procedures.rs:2548-2597 and 2156-2257).  The reference
 * issues no LAGraph call here and its tie-breaks are accidents of its heap order; these are the rules:
 *   - W is square; W(u, v) is the weight of the arc u -> v.  A valued snapshot holds one IEEE-754 binary64 BIT PATTERN per
 *     entry in its uint64 value; a BOOL snapshot means every weight is 1.0.  A hypersparse W is accepted;
 *   - a diagonal entry is ignored; there is no active bitmap: the caller compacts the node ids;
 *   - -0.0 is 0.0.  A NaN, or a weight with the sign bit set other than -0.0, anywhere in W is FGPU_INVALID (one reduction
 *     pass before the search);
 *   - a relaxation whose sum dist[u] + w is not finite is skipped (the reference's !far_weight.is_finite()): a +inf entry is
 *     never used, and neither is a route whose length overflows.
 * dist[nrows] (a HOST array; a pinned one — fgpu_host_alloc — is filled by DMA, as fgpu_bfs' level[]): dist[src] = +0.0,
 * +inf for the vertices no route reaches, otherwise the minimum over all src -> v routes of the route's weights added left
 * to right from the source in FP64.  fl(a + w) is monotone in a for w >= 0, so this value is unique: it is what a heap
 * Dijkstra computes, bit for bit, and identical from run to run and under every bucket width.
 * parent[nrows] (nullable HOST array; -1 = unreached, parent[src] = src) is a pure function of dist and W.  An entry (u, v),
 * u != v, is TIGHT when dist[u] + W(u, v) is finite and equals dist[v].  depth[v] is the BFS depth of v from src over the tight
 * entries alone; parent[v] is the smallest u with (u, v) tight and depth[u] + 1 == depth[v].  The tight entries span every
 * reached vertex (a Dijkstra tree consists of them), so the parent chains form a tree rooted at src, whatever zero-weight
 * cycles or absorbed weights (1.0 + 1e-20 == 1.0) W holds.  The parent search is skipped when parent and stats are both NULL.
 * stats (nullable): [0] relaxation launches that had work, [1] vertices taken off a worklist, re-insertions counted (divided
 * by the reached vertices: the work efficiency), [2] entries read (both phases), [3] the deepest depth.
 * The bucket width is a power of two derived on the device from the mean finite weight and the mean degree (1.0 for a BOOL
 * W); fgpu_set_option "sssp_delta_log2" = -1074 .. 1023 forces 2^value, 4096 (the default) restores the derived width;
 * fgpu_get_option reads it back, and "sssp_last_delta_log2" is the width the last call used (1024: one bucket for all).
 * Errors: NULL ctx / W / dist: FGPU_NULL_POINTER; non-square W: FGPU_DIM_MISMATCH; src >= nrows: FGPU_OUT_OF_BOUNDS;
 * nrows >= 2^32 - 1: FGPU_INVALID.  nrows == 0 is a no-op.  The step loop (a relaxation of the near pile, or a move to the
 * next non-empty bucket) has a hard cap of 4 (n^2 + n) + 64 steps — every vertex enters a bucket once and a bucket is a
 * fixed point within n relaxations, so a correct run stays below n^2 + 2 n — past which the call returns FGPU_INVALID with a
 * message instead of running on. */
fgpu_info fgpu_sssp(fgpu_ctx* ctx, const fgpu_mat* W, uint64_t src, double* dist, int64_t* parent, uint64_t stats[4]);

/* The hop-bounded shortest-path table from one source: what prunes algo.SPpaths' enumeration shapes (enumerate_paths,
 * algo_procedures.rs:2405-2514, walks every simple path under its weight bound; whether a prefix can still END at the target
 * within maxLen arcs is the cheapest way from the target in at most r arcs over the transposed weights, which is this table).
 * The reference has no counterpart; these are the rules:
 *   - W follows fgpu_sssp's rules exactly: square, W(u, v) the weight of the arc u -> v as a binary64 bit pattern, a BOOL
 *     snapshot means every weight is 1.0, a hypersparse W is accepted, a diagonal entry is ignored, -0.0 is 0.0, a NaN or a
 *     negative weight anywhere in W is FGPU_INVALID, a relaxation whose sum is not finite is skipped;
 *   - max_hops is 0 .. FGPU_SSSP_HOPS_MAX.
 * table[(max_hops + 1) * nrows] (a HOST array; a pinned one — fgpu_host_alloc — is filled by DMA): table[h * nrows + v] =
 * D_h[v], with D_0[src] = +0.0 and +inf elsewhere, and
 *   D_h[v] = min(D_{h-1}[v], min over the entries (u, v), u != v, of fl(D_{h-1}[u] + W(u, v)) where that sum is finite).
 * fl(a + w) is monotone in a for w >= 0, so D_h[v] is the minimum over all routes src -> v of at most h arcs of the route's
 * weights added left to right from the source in FP64: unique, and identical from run to run.  A round reads D_{h-1} only —
 * one round never travels two arcs.  Once a round lowers nothing, every later row repeats the last one.
 * stats (nullable): [0] rounds whose frontier (the vertices the round before lowered; round 1: src) was not empty,
 * [1] frontier entries taken over all rounds (a vertex is in a frontier once per round), [2] entries read, [3] the first h in
 * 1 .. max_hops with D_h == D_{h-1} everywhere, max_hops + 1 if there is none.
 * Errors: NULL ctx / W / table: FGPU_NULL_POINTER; non-square W: FGPU_DIM_MISMATCH; max_hops outside 0 .. FGPU_SSSP_HOPS_MAX,
 * nrows >= 2^32 - 1: FGPU_INVALID; src >= nrows: FGPU_OUT_OF_BOUNDS.  nrows == 0 is a no-op. */
#define FGPU_SSSP_HOPS_MAX 32
fgpu_info fgpu_sssp_hops(fgpu_ctx* ctx, const fgpu_mat* W, uint64_t src, int32_t max_hops, double* table, uint64_t stats[4]);

/* The shortest-path DAG between two bound vertices: the numeric core of the reference's AllShortestPathsOp
 * (runtime/ops/all_shortest_paths.rs:128-267, MATCH p = allShortestPaths((a)-[*]->(b))).  The reference runs a hash-map BFS per
 * input row and a lazy DFS over the recorded predecessors; the DFS touches exactly the pairs returned here.
 *   - A is the pattern of a square adjacency (values are ignored, a hypersparse A is accepted), At its transpose or NULL: the
 *     call then builds the transpose for its own use and releases it.  Nothing is cached on either matrix.  An undirected
 *     pattern -[*]- is the caller passing S = A U A' for both;
 *   - max_hops < 0 is unbounded; max_hops == 0 gives no path;
 *   - src != dst: L = the BFS distance from src to dst over A if it is at most max_hops (the reference's min_hops is always 1
 *     here: cypher.rs:1324-1331).  Self-loops never matter;
 *   - src == dst, the cycle shape (:209-235): L = 1 + the least d(src, u) over the in-neighbours u of src, u = src at distance
 *     0 when src has a self-loop.  Over a symmetric pattern a single edge therefore closes a cycle of length 2, as the
 *     reference's reuse of an edge in both directions does; there is no trail check.
 * *length = L, or -1 when there is no path within the bound; then *n_pairs = 0 and the three arrays are NULL.  Otherwise
 * from / to / depth (fgpu_free each) hold the *n_pairs pairs (u, v) with an entry u -> v and d(src, u) + 1 + d(v, dst) = L —
 * in the cycle shape d(v, dst) = 0 for the closing pairs (u, src) — in ascending (from, to) order, each once, and
 * depth[k] = d(src, from[k]) in 0 .. L - 1.  Repeated calls give identical arrays.
 * The search is bidirectional and level-synchronous: it grows the ball whose frontier has fewer entries to scan, a whole level
 * at a time, and stops at the first level whose new vertices the other ball already holds (spdag.hip).  The option spdag_sides:
 * 0 that rule, 1 forward only, 2 backward only, 3 strict alternation starting forward; every setting returns the same length
 * and arrays.
 * stats (nullable): [0] forward levels expanded, [1] backward levels expanded (the cycle shape's first one included),
 * [2] vertices claimed forward, [3] vertices claimed backward (seeds not counted), [4] entries scanned by the expansions,
 * [5] entries scanned by the sweeps that collect the DAG, [6] meeting vertices, [7] DAG vertices (the cycle shape counts src
 * at both ends).  [5] and [7] stay 0 without a path.
 * Errors: NULL ctx / A / output pointer: FGPU_NULL_POINTER; non-square A or an At of other dimensions: FGPU_DIM_MISMATCH;
 * src or dst >= nrows: FGPU_OUT_OF_BOUNDS; nrows >= 2^32 - 1 or nnz >= 2^32 - 1: FGPU_INVALID.  nrows == 0 gives no path.
 * The call runs on the calling thread's lane: concurrent callers on the same matrices are independent. */
fgpu_info fgpu_shortest_dag(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, uint64_t src, uint64_t dst, int64_t max_hops,
                            int64_t* length, uint64_t* n_pairs, uint64_t** from, uint64_t** to, uint64_t** depth,
                            uint64_t stats[8]);

/* fgpu_shortest_dag for a whole batch of queries over one adjacency: what an AllShortestPathsOp fed a parent batch of rows asks
 * for.  The single call is bound by its launches and counter read-backs, not by its work; here `slots` queries at a time advance
 * in lock-step rounds and share every round's launches and its one read-back (spdag_batch.hip).
 *   - query i is (src[i], dst[i]) under the one max_hops of the call; A, At and max_hops mean what they mean above;
 *   - length[i] is what fgpu_shortest_dag returns for query i, -1 without a path;
 *   - pair_off has count + 1 entries, pair_off[0] = 0: the slice pair_off[i] .. pair_off[i + 1] of from / to / depth holds
 *     exactly the single call's three arrays for query i, in its order.  A query without a path has an empty slice;
 *   - stats (nullable, count * 8 words): stats[8 i .. 8 i + 8) are the single call's stats for query i.  Every query picks its
 *     side by the single call's rule from its own frontier counts (the cycle shape keeps its first backward expansion), so this
 *     holds under every spdag_sides setting, with At given or NULL;
 *   - the queries are independent: duplicates and any order are allowed, and permuting the queries permutes the output;
 *   - from / to / depth are freed with fgpu_free each; they are NULL when pair_off[count] == 0.  count == 0 returns FGPU_OK with
 *     pair_off[0] = 0.  Repeated calls give identical arrays.
 * slots is the number of queries searched together, at most FGPU_SPDAG_SLOTS_MAX.  Every slot has dense level words and mark
 * bits of its own, 8 nrows + nrows / 4 bytes; every other temporary grows with the entries scanned.  slots = 0 derives it:
 * min(count, FGPU_SPDAG_SLOTS_MAX, max(1, 2 GiB / (8 nrows))) — the level words of a group stay within 2 GiB, which is 64 slots
 * up to 2^22 vertices.  The result does not depend on slots.
 * A missing At is built once per call and released with it; nothing is cached on either matrix.
 * Errors: NULL ctx / A / length / pair_off / from / to / depth, or NULL src / dst with count > 0: FGPU_NULL_POINTER; non-square
 * A or an At of other dimensions: FGPU_DIM_MISMATCH; slots > FGPU_SPDAG_SLOTS_MAX, nrows >= 2^32 - 1 or nnz >= 2^32 - 1:
 * FGPU_INVALID; any src[i] or dst[i] >= nrows: FGPU_OUT_OF_BOUNDS for the whole call, before any work — the message names i,
 * no output is written or allocated.  nrows == 0 gives no path for every query.
 * The call runs on the calling thread's lane: concurrent callers on the same matrices are independent. */
#define FGPU_SPDAG_SLOTS_MAX 64
fgpu_info fgpu_shortest_dag_batch(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* src, const uint64_t* dst,
                                  uint64_t count, int64_t max_hops, uint32_t slots, int64_t* length, uint64_t* pair_off,
                                  uint64_t** from, uint64_t** to, uint64_t** depth, uint64_t* stats);

/* shortestPath((a)-[:T*..k]->(b)) for a whole batch of bound pairs: the ONE path the reference's per-row bidirectional search
 * returns (runtime/eval.rs:1386-1513, bfs_shortest_path, over the neighbour streams of eval.rs:140-244), to the vertex.
 * fgpu_shortest_dag_batch cannot serve it: which of several shortest paths comes back is fixed by the order of the frontiers, by
 * the side that grows and by the first discoverer of every vertex, and this call keeps all three (spath_batch.hip).
 * Neighbours.  neighbors(v) of a side is the set of columns of row v of its pattern, ascending, each once.  The forward side
 * reads F, the backward side reads B: for a directed pattern F is the union of the types' matrices (the adjacency when no type
 * is named) and B its transpose — B == NULL builds the transpose for the call and releases it with it; for an undirected
 * pattern the caller passes S = F U F' for both.  Values are ignored, hypersparse patterns are accepted, nothing is cached on
 * either matrix.
 * Start.  src == dst gives no path (the caller serves the single-node path of min_hops == 0 itself).  Each ball starts as its
 * seed at depth 0, each frontier as its seed, df = db = 0.
 * A round.
 *   1. If either frontier is empty, or df + db >= max_hops (max_hops < 0: unbounded; 0: no path), there is no path.
 *   2. The forward side expands iff it has at most as many frontier VERTICES as the backward side (not entries).
 *   3. The expanding side walks its frontier in frontier order and each row in ascending column order; the position of an
 *      entry in that concatenation is its key.
 *   4. A vertex not yet in the side's own ball is claimed by the smallest key that reaches it: its parent is the frontier
 *      vertex of that key's row, its depth the side's depth + 1.
 *   5. A claimed vertex that the other ball already holds is a meeting candidate; the other claimed vertices form the side's
 *      next frontier, in ascending key order.
 *   6. The level always runs to its end, and the side's depth grows by one.
 *   7. With candidates, the meeting vertex is the candidate of the least other-side depth, then of the least key, and the
 *      search ends.
 * Result.  The forward parents from the meeting vertex back to src, reversed, then the backward parents on to dst:
 * length + 1 node ids.
 *   - length[i] is the edge count of query i's path, -1 without one;
 *   - node_off has count + 1 entries, node_off[0] = 0: nodes[node_off[i] .. node_off[i + 1]) is the path of query i, empty
 *     without one.  *nodes is NULL when node_off[count] == 0, else freed with fgpu_free;
 *   - stats (nullable, count * 8 words) of query i: [0] forward levels, [1] backward levels, [2] vertices claimed forward,
 *     [3] vertices claimed backward (seeds not counted, candidates counted), [4] entries walked, [5] the meeting vertex or
 *     2^64 - 1, [6] meeting candidates of the last level (0 without a path), [7] 0;
 *   - the queries are independent: duplicates and any order are allowed.  The result does not depend on slots, on the calling
 *     thread or on the run.
 * slots is the number of queries searched together, at most FGPU_SPATH_SLOTS_MAX.  Every slot has a dense claim word and a
 * parent per vertex and side, 24 nrows bytes; every other temporary grows with the entries walked.  slots = 0 derives it:
 * min(count, FGPU_SPATH_SLOTS_MAX, max(1, 2 GiB / (24 nrows))).
 * Errors: NULL ctx / F / length / node_off / nodes, or NULL src / dst with count > 0: FGPU_NULL_POINTER; non-square F or a B of
 * other dimensions: FGPU_DIM_MISMATCH; slots > FGPU_SPATH_SLOTS_MAX, nrows >= 2^32 - 1 or nnz >= 2^32 - 1: FGPU_INVALID; any
 * src[i] or dst[i] >= nrows: FGPU_OUT_OF_BOUNDS for the whole call, before any work — the message names i, no output is written
 * or allocated.  count == 0 returns FGPU_OK with node_off[0] = 0; nrows == 0 gives no path for every query.
 * The call runs on the calling thread's lane: concurrent callers on the same matrices are independent. */
#define FGPU_SPATH_SLOTS_MAX 64
fgpu_info fgpu_shortest_path_batch(fgpu_ctx* ctx, const fgpu_mat* F, const fgpu_mat* B, const uint64_t* src, const uint64_t* dst,
                                   uint64_t count, int64_t max_hops, uint32_t slots, int64_t* length, uint64_t* node_off,
                                   uint64_t** nodes, uint64_t* stats);

/* Exhaustive vector similarity search: the numeric core of db.idx.vector.queryNodes / queryRelationships
 * (runtime/ops/node_by_vector_scan.rs, edge_by_vector_scan.rs) and of vec.euclideanDistance / vec.cosineDistance.  The
 * reference asks an approximate HNSW graph (RediSearch / VecSim, index/mod.rs:1768-1823) for k candidates, recomputes each
 * candidate's distance from the stored vector and sorts the survivors (graph.rs:3408-3457, runtime/vec_distance.rs), one
 * query per parent row.  Here every stored vector is scored against a whole batch of queries, so recall is 1 by
 * construction; RediSearch's source is not vendored, these are the rules:
 *   - an index holds vectors of one dimension dim = 1 .. FGPU_VECIDX_DIM_MAX under one metric, each under an id below
 *     2^32 - 1 (a larger id is FGPU_INVALID).  The store is a dense array on the device without holes; its capacity doubles;
 *   - fgpu_vecidx_set is an upsert of n (id, vector) pairs: a present id is replaced, and of an id given twice in one call
 *     the last occurrence wins.  fgpu_vecidx_remove moves the last vector into each hole; an absent id is not an error and
 *     *removed (nullable) counts the ids that were present.  fgpu_vecidx_get copies one stored vector out (*present = 0: no
 *     such id, vec untouched);
 *   - a component that is NaN or +-inf, in fgpu_vecidx_set or in a query, is FGPU_INVALID and the call changes nothing.  The
 *     reference would sort such rows arbitrarily; refusing them is what makes the order below total;
 *   - the reported distance D(q, x) is computed in FP64 from the stored f32 components, accumulated in index order, for the
 *     returned entries only, as vec_distance.rs does:
 *       euclidean  sqrt(sum (q_i - x_i)^2)
 *       ip         -sum q_i x_i
 *       cosine     1 - sum q_i x_i / (sqrt(sum q_i^2) * sqrt(sum x_i^2)), and exactly 1.0 when either vector is all zeros;
 *   - the SELECTION key is f32.  S(q, x) is the dot product as a k-ordered fmaf chain from 0 over i = 0 .. dim - 1 — what
 *     v_mfma_f32_16x16x4_f32 produces bit for bit, and no kernel splits K across lanes or wavefronts; nx and nq are the same
 *     chain of x . x and q . q.  Then
 *       euclidean  key = fl(fl(nq + nx) - 2 S)
 *       ip         key = -S
 *       cosine     key = fl(1 - fl(S / fl(fl(sqrt(nq)) * fl(sqrt(nx))))), sqrt and the division correctly rounded, and 1.0
 *                  when nq or nx is 0.
 *     The key is a pure function of (q, x): the same for a query alone and for that query inside a batch of 1024.  Keys are
 *     compared as f32 values with -0.0 = +0.0.  Finite components can still overflow f32 on the way (components near 1e19
 *     and beyond under euclidean: nq, nx or S becomes inf; a cosine denominator that underflows to 0): a key of -inf or +inf
 *     orders as the f32 value it is, and a NaN key (inf - inf, 0 / 0) sorts after every other key, +inf included.  The chain
 *     itself never gives a NaN: fmaf(a, b, +-inf) with finite a and b adds the exact, finite product and is that infinity, so
 *     an S that overflowed keeps its sign, and under ip every key is a number or -inf or +inf.  With the id as the second
 *     component the order is total for every input the calls accept; D is FP64 and does not overflow;
 *   - fgpu_vecidx_knn returns, per query, the kk = min(k, count) entries of smallest (key, id), in ascending (D, id) order:
 *     *kk_out = kk, and ids / dist (HOST arrays of nq * kk) have row stride kk.  The caller sizes them from fgpu_vecidx_info.
 *     k == 0 is FGPU_INVALID.  With nq == 0 or count == 0, kk is 0 and the call does nothing (ids / dist may be NULL);
 *   - stats (nullable): [0] scoring launches, [1] query tiles of 16 (padding tiles included), [2] bytes of stored vectors
 *     read by scoring, [3] entries whose key tied the kk-th key where more of them tied than places were left, so that the id
 *     order had to decide;
 *   - a NULL ctx / index / required array is FGPU_NULL_POINTER;
 *   - fgpu_vecidx_set, _remove and _free must not run concurrently with any other call on the same index (the reference
 *     holds the graph's write lock there); fgpu_vecidx_knn / _get / _info calls from several threads on one index are
 *     independent, each on its caller's lane.
 * One scoring kernel family serves every nq: the queries are padded to tiles of 16, one reading of the store serves up to 64
 * of them, and the key images of a chunk of queries go through a radix select on the device; only the final (D, id) ordering
 * of the kk survivors of a query happens on the host (vecidx.hip).  A chunk is as many queries (16, 32 or a multiple of 64, at
 * most 4096) as keep the key images (4 bytes per query and stored vector) and the survivors (20 bytes per query and returned
 * entry) under 256 MiB of device scratch each — never fewer than one tile of 16, whatever that takes. */
typedef struct fgpu_vecidx fgpu_vecidx;
#define FGPU_VEC_EUCLIDEAN 0
#define FGPU_VEC_COSINE 1
#define FGPU_VEC_IP 2
#define FGPU_VECIDX_DIM_MAX 4096
fgpu_info fgpu_vecidx_new(fgpu_ctx* ctx, fgpu_vecidx** out, uint32_t dim, int metric);
fgpu_info fgpu_vecidx_free(fgpu_vecidx* index);
fgpu_info fgpu_vecidx_info(const fgpu_vecidx* index, uint32_t* dim, int* metric, uint64_t* count);
fgpu_info fgpu_vecidx_set(fgpu_ctx* ctx, fgpu_vecidx* index, const uint64_t* ids, const float* vecs /* n * dim */, uint64_t n);
fgpu_info fgpu_vecidx_remove(fgpu_ctx* ctx, fgpu_vecidx* index, const uint64_t* ids, uint64_t n, uint64_t* removed);
fgpu_info fgpu_vecidx_get(fgpu_ctx* ctx, const fgpu_vecidx* index, uint64_t id, float* vec /* dim */, int* present);
fgpu_info fgpu_vecidx_knn(fgpu_ctx* ctx, const fgpu_vecidx* index, const float* queries /* nq * dim */, uint64_t nq, uint64_t k,
                          uint64_t* ids /* nq * kk */, double* dist /* nq * kk */, uint64_t* kk_out, uint64_t stats[4]);

/* The smallest stored value of A under the order of fgpu_msf's K (the IEEE totalOrder with -0.0 = +0.0), as a binary64 bit
 * pattern (LAGraph_Cached_EMin).  *found = 0 when A has no entry; a BOOL snapshot answers 1.0.  A device reduction: no entry
 * visits the host. */
fgpu_info fgpu_mat_min_val(fgpu_ctx* ctx, const fgpu_mat* A, uint64_t* bits, int* found);

/* Betweenness centrality (batched Brandes): replaces LAGr_Betweenness(&centrality, G, sources, ns, msg) as called by
 * algo.betweenness (algo_procedures.rs:884-1017; binding lagraph_bindings.rs:539-546).  centrality[v] = the sum over the
 * sources s of delta_s(v) = sum over out-neighbours w of v with d_s(w) = d_s(v) + 1 of sigma_s(v) / sigma_s(w) * (1 + delta_s(w)),
 * sigma the number of shortest directed paths over A's out-edges, d the BFS depth.  A source never scores for itself; a
 * duplicate source counts twice; nsrc == 0 gives all zeros; scores are not normalised.  `At` (nullable) is A's transpose —
 * NULL uses the snapshot's cached transpose (built on first use).  `active_bitmap` (nullable, nrows bits, as fgpu_pagerank)
 * restricts the run to the induced subgraph of the flagged vertices; the other slots get 0.  centrality[nrows] is a HOST
 * array (filled by DMA when pinned — fgpu_host_alloc — by staging otherwise).  stats (nullable): [0] batches, [1] forward
 * levels expanded, summed over batches, [2] adjacency entries read (forward and backward), [3] deepest level.  Errors: NULL
 * A / centrality, or NULL sources with nsrc > 0: FGPU_NULL_POINTER; non-square A or a mismatched At: FGPU_DIM_MISMATCH; a
 * source >= nrows: FGPU_OUT_OF_BOUNDS; a source outside active_bitmap: FGPU_INVALID.  Options "bc_batch", "bc_direction".
 * Repeated calls and every bc_direction give bit-identical output.  nrows == 0 is a no-op. */
fgpu_info fgpu_betweenness(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                           const uint64_t* sources, uint64_t nsrc, double* centrality, uint64_t stats[4]);

/* Level-synchronous BFS: replaces LAGr_BreadthFirstSearch_Extended(level, parent, G,
 * src, max_level, -1, false) as called by algo.BFS (algo_procedures.rs:1079-1088;
 * binding lagraphx_bindings.rs:585-594).  level[n] (int32, -1 = unreached, source = 0),
 * parent[n] (nullable, int64, -1 = none, parent[src] = src) are HOST arrays (pinned ones — fgpu_host_alloc — are
 * filled by DMA: 0.3 ms for the 16 MiB level[] of RMAT-22 instead of 0.9 ms through staging into pageable memory).
 * max_level < 0 => unlimited.  At may be NULL (push only).  edges_traversed
 * (nullable) = sum of out-degrees of reached vertices (TEPS numerator).
 * The search plan of the last call over the same (A, At) pair stays attached to A (released with either matrix, rebuilt
 * after fgpu_set_option), so repeated calls pay the search and the 4 N-byte copy-out, not plan creation. */
fgpu_info fgpu_bfs(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, uint64_t src,
                   int64_t max_level, int32_t* level, int64_t* parent,
                   uint64_t* edges_traversed);

/* Plan API: keeps the BFS workspace resident so repeated searches (bench steps,
 * many roots) pay no allocation, and results can stay on device.
 * Column-slab partition for multi-GPU: rank `rank` of `nranks`
 * owns destination vertices [rank*slab, (rank+1)*slab), slab = ceil(n/nranks)
 * rounded up to 4096; A / At passed here are the rank's slab (A restricted to the
 * owned columns, At restricted to the owned rows, both with GLOBAL ids).
 * nranks == 1 is the plain single-GPU case. */
fgpu_info fgpu_bfs_plan_create(fgpu_ctx* ctx, fgpu_bfs_plan** plan, const fgpu_mat* A,
                               const fgpu_mat* At, int rank, int nranks);
fgpu_info fgpu_bfs_plan_free(fgpu_bfs_plan* plan);
/* Tunables: alpha/beta of the push<->pull switch (Beamer), 0 keeps defaults;
 * force_direction 0 auto / 1 push only / 2 pull only. */
fgpu_info fgpu_bfs_plan_tune(fgpu_bfs_plan* plan, double alpha, double beta, int force_direction);
/* Run one whole BFS on a single-rank plan; results stay on device. */
fgpu_info fgpu_bfs_run(fgpu_bfs_plan* plan, uint64_t src, int64_t max_level, int want_parent);
/* The same search without the final host wait: clears the workspace, seeds `src` and enqueues
 * `levels` (<= 0: 10) level kernels on the ctx stream; kernels past the last level are no-ops.
 * fgpu_bfs_wait() returns once the search has ended (it enqueues more levels if `levels` was too
 * few).  Two plans over the same matrices let the host enqueue search i+1 while search i runs. */
fgpu_info fgpu_bfs_run_async(fgpu_bfs_plan* plan, uint64_t src, int64_t max_level, int want_parent,
                             int levels);
fgpu_info fgpu_bfs_wait(fgpu_bfs_plan* plan);
/* Copy results of the last run to host (either pointer may be NULL). */
fgpu_info fgpu_bfs_fetch(fgpu_bfs_plan* plan, int32_t* level, int64_t* parent);
/* Stats of the last run: stats[0]=levels, [1]=reached vertices (incl. source),
 * [2]=edges traversed (sum outdeg of reached), [3]=push levels, [4]=pull levels,
 * [5]=edges scanned by push kernels, [6]=edges scanned by pull kernels. */
fgpu_info fgpu_bfs_stats(fgpu_bfs_plan* plan, uint64_t stats[8]);

/* Multi-rank stepping (driven by the host loop that owns the collective):
 *   begin(src) ; repeat { step() ; <allgather slab words> ; commit() } until done.
 * local_words / global_words are DEVICE pointers owned by the plan:
 *   local  = this rank's new-frontier slab: slab/64 bitmap words + 2 stat words
 *            (count, sum of out-degrees) => `words_per_rank` uint64 each;
 *   global = nranks * words_per_rank, the allgather destination. */
fgpu_info fgpu_bfs_part_buffers(fgpu_bfs_plan* plan, void** local_words, void** global_words,
                                uint64_t* words_per_rank);
/* Let the caller own the exchange buffers instead (e.g. torch tensors handed to
 * torch.distributed.all_gather_into_tensor): local = words_per_rank uint64, global =
 * nranks * words_per_rank uint64, both DEVICE memory that outlives the plan's use.  Both are
 * zeroed by the call. */
fgpu_info fgpu_bfs_part_set_buffers(fgpu_bfs_plan* plan, void* local_words, void* global_words);
fgpu_info fgpu_bfs_part_begin(fgpu_bfs_plan* plan, uint64_t src, int64_t max_level);
fgpu_info fgpu_bfs_part_step(fgpu_bfs_plan* plan);
fgpu_info fgpu_bfs_part_commit(fgpu_bfs_plan* plan);
/* Non-blocking-ish poll of the device control block (one small D2H): done != 0 when
 * the last committed frontier was empty or max_level was reached. */
fgpu_info fgpu_bfs_part_done(fgpu_bfs_plan* plan, int32_t* done, int32_t* level);

/* Fused slab path (multi-rank v2): ONE level kernel and ONE frontier all-gather per level — no commit pass,
 * no control kernel.  The rank owns destinations [lo, hi) exactly as above; because a column slab only ever
 * discovers vertices it owns, the level kernel updates visited / level / parent at discovery and writes its
 * owned words of the next frontier into a send buffer; the host all-gathers that buffer into `global_words`
 * (nranks * words_per_rank uint64 = the global frontier bitmap) and launches the next level.  Everything a
 * level needs from other ranks is that bitmap: termination comes from its population (identical on all
 * ranks), the push / pull choice is each rank's own.
 *   set_buffers : send0 / send1 (words_per_rank uint64 each, double-buffered) and global_words, caller-owned
 *                 DEVICE memory (torch tensors handed to all_gather_into_tensor);
 *   set_degrees : optional global out-degree of every vertex (uint32[n], device) so that the owner accounts a
 *                 vertex's whole out-degree in edges_traversed (a column slab holds only its share);
 *   begin       : clears the workspace and seeds `src` on every rank (no collective for level 0);
 *   level       : enqueues one level; *send_index (0/1) = the send buffer to all-gather next;
 *   fgpu_bfs_part_done / _stats / _fetch work as for the stepped path (reached / edges_traversed are the
 *   rank's own share: sum them over ranks). */
fgpu_info fgpu_bfs_slab_set_buffers(fgpu_bfs_plan* plan, void* send0, void* send1, void* global_words);
fgpu_info fgpu_bfs_slab_set_degrees(fgpu_bfs_plan* plan, const uint32_t* global_out_degrees);
fgpu_info fgpu_bfs_slab_begin(fgpu_bfs_plan* plan, uint64_t src, int64_t max_level, int want_parent);
fgpu_info fgpu_bfs_slab_level(fgpu_bfs_plan* plan, int* send_index);
/* deg[r] = stored entries of row r (DEVICE uint32[nrows]); summed over the ranks' column slabs it is the global
 * out-degree vector fgpu_bfs_slab_set_degrees takes. */
fgpu_info fgpu_mat_row_degrees(fgpu_ctx* ctx, const fgpu_mat* a, uint32_t* out_dev);

/* Build this rank's column slab of a full matrix: out = A[:, lo:hi) (global ids
 * kept), and its transpose restricted to rows [lo,hi).  Used to shard a replicated
 * or host-loaded adjacency. */
fgpu_info fgpu_mat_col_slab(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a, uint64_t lo,
                            uint64_t hi);
fgpu_info fgpu_mat_row_slab(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a, uint64_t lo,
                            uint64_t hi);

/* ---- multi-GPU: RCCL communicator + in-library partitioned BFS -------------------------
 * The reference reaches its BFS through one call (LAGr_BreadthFirstSearch_Extended, algo_procedures.rs:1079-1088);
 * a process that links this library reaches the multi-GPU form the same way: the communicator, the level loop and
 * the frontier exchange (an all-gather-v: grouped ncclSend / ncclRecv to every peer, one xGMI link per piece) are
 * inside libfgpu.so.
 *   one process per GPU : rank 0 calls fgpu_comm_unique_id, the launcher's own channel carries the 128 bytes,
 *                         every rank calls fgpu_comm_init_rank on its context;
 *   one process, N GPUs : one context per device, fgpu_comm_init_all (ncclCommInitAll) — the Redis-module form. */
#define FGPU_COMM_ID_BYTES 128
fgpu_info fgpu_comm_unique_id(uint8_t* id /* FGPU_COMM_ID_BYTES */);
fgpu_info fgpu_comm_init_rank(fgpu_ctx* ctx, int nranks, int rank, const uint8_t* id);
fgpu_info fgpu_comm_init_all(fgpu_ctx* const* ctxs, int n);
fgpu_info fgpu_comm_finalize(fgpu_ctx* ctx);
fgpu_info fgpu_comm_info(fgpu_ctx* ctx, int32_t* rank, int32_t* nranks);
/* nnz-balanced slab boundaries of the destination vertices (= columns of A): splits[0] = 0, splits[nparts] = the
 * vertex count rounded up to 4096, every boundary a multiple of 4096, part k holding ~ nnz / nparts of A's entries
 * (prefix sum of in-degrees; R-MAT skew otherwise overloads the parts that own the hubs). */
fgpu_info fgpu_mat_balanced_splits(fgpu_ctx* ctx, const fgpu_mat* a, int nparts, uint64_t* splits /* nparts + 1 */);
/* The partition arithmetic on its own — pure host functions (no device, no context), so that a launcher, the host layer and
 * the CPU tests all use the ONE definition the level loop uses:
 *   fgpu_splits_shift             log2 of the column-block width fgpu_mat_balanced_splits histograms with (>= 12);
 *   fgpu_balanced_splits_from_hist the boundary choice from per-block entry counts (the host half of the call above);
 *   fgpu_slab_layout              rank r's vertex range [lo, hi) and its words (offset, count) in the global frontier
 *                                 bitmap = what the per-level all-gather-v moves; splits == NULL: the equal slabs of
 *                                 fgpu_bfs_plan_create (ceil(n / nranks) rounded up to 4096).  Outputs are nullable. */
uint32_t fgpu_splits_shift(uint64_t ncols);
fgpu_info fgpu_balanced_splits_from_hist(const uint64_t* block_counts, uint64_t nblocks, uint32_t shift, uint64_t ncols,
                                         int nparts, uint64_t* splits /* nparts + 1 */);
fgpu_info fgpu_slab_layout(const uint64_t* splits /* nullable: nranks + 1 */, uint64_t n, int nranks, uint64_t* lo,
                           uint64_t* hi, uint64_t* word_off, uint64_t* word_cnt);
/* fgpu_bfs_plan_create with caller-chosen slab boundaries: rank owns destinations [splits[rank], splits[rank+1]);
 * A_slab = A[:, slab], At_slab = A'[slab, :] (fgpu_mat_col_slab + fgpu_mat_transpose), global ids. */
fgpu_info fgpu_bfs_plan_create_slab(fgpu_ctx* ctx, fgpu_bfs_plan** plan, const fgpu_mat* A_slab,
                                    const fgpu_mat* At_slab, int rank, int nranks, const uint64_t* splits);
/* One whole search over the partition: per level one kernel per rank and one frontier exchange.  `plans` = this
 * process' ranks: ONE plan when every GPU has its own process (exchange over the context's communicator), ALL plans
 * in rank order when one process drives the node (RCCL if the contexts were joined by fgpu_comm_init_all, event-ordered
 * peer copies otherwise).  Results per rank through fgpu_bfs_fetch (the owned range) / fgpu_bfs_stats (the rank's
 * share of reached / edges_traversed: sum over ranks). */
fgpu_info fgpu_bfs_dist_run(fgpu_bfs_plan* const* plans, int nplans, uint64_t src, int64_t max_level,
                            int want_parent);
/* Time split of the plan's last fgpu_bfs_dist_run: HIP-event sums over its level kernels and over its exchanges
 * (an exchange includes the wait for the slowest rank) — zero unless the "dist_timing" option was on during the run —
 * and the number of level launches. */
fgpu_info fgpu_bfs_dist_times(fgpu_bfs_plan* plan, double* level_ms, double* collective_ms, uint64_t* launches);

/* ---- measurement hooks (bench.py; not reference APIs) --------------------- */

/* Time `iters` launches of one named kernel with HIP events on the ctx stream.
 * which: 0 = full-pass boolean pull SpMV over the CSR of the matrix passed (dense frontier, no
 * mask, no early exit), 1 = push over A with a dense frontier, 2 = the same full pass as 0 over
 * the LDS-tile layout (the "RMAT-22 boolean SpMV" roofline case), 3 = as 2 with the caches flushed before every timed
 * launch (a 512 MiB scratch buffer is read between launches: the 256 MiB Infinity Cache holds none of the
 * layout when the pass starts, and no write-back is pending).  Returns avg ms per launch and algorithmic bytes per launch
 * (SURVEY.md §8d formulas). */
fgpu_info fgpu_bench_spmv(fgpu_ctx* ctx, const fgpu_mat* A, int which, int iters,
                          double* avg_ms, uint64_t* alg_bytes);
/* Context-wide kernel profiler for the non-BFS paths (k-hop products, merges, transposes): while enabled, every
 * launch of a modelled kernel is bracketed by HIP events on its lane's stream.  fgpu_prof_read synchronises,
 * folds the records by kernel name (static strings), returns total ms / launch count / algorithmic bytes
 * (SURVEY.md §8d accounting; 0 = not modelled) per name and clears them.  Enabling clears earlier records. */
fgpu_info fgpu_prof_enable(fgpu_ctx* ctx, int enable);
fgpu_info fgpu_prof_read(fgpu_ctx* ctx, const char** names, double* ms, uint64_t* launches,
                         uint64_t* alg_bytes, int cap, int* n);
/* Uniform sample of the stored entries of `a` (bench / test data for "0.1 % random tombstones"):
 * (r, c) is kept iff mix64(seed ^ mix64(r << 32 | c)) % denom == 0, mix64 = the splitmix64 finaliser — a function
 * of the coordinate, so a CPU model draws the same sample.  Pattern only.  Not a reference API. */
fgpu_info fgpu_mat_sample(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* a, uint64_t seed, uint32_t denom);
/* Per-kernel accumulated HIP-event timings of a plan (enabled by
 * fgpu_bfs_plan_profile(plan,1)): names[i] (static strings), ms[i], launches[i],
 * alg_bytes[i]; returns count in *n (<= cap). */
fgpu_info fgpu_bfs_plan_profile(fgpu_bfs_plan* plan, int enable);
fgpu_info fgpu_bfs_plan_profile_read(fgpu_bfs_plan* plan, const char** names, double* ms,
                                     uint64_t* launches, uint64_t* alg_bytes, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif /* FGPU_H */
