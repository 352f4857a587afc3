/*
 * falkor_host.h — C surface of the C++ host layer (falkordb_amd/host/, libfalkor_host.so).
 *
 * The host layer is the C++17 stand-in for the Rust code that sits between FalkorDB's execution-plan
 * operators and the GraphBLAS boundary (Matrix<T>, VersionedMatrix, Tensor, the traversal slice of Graph,
 * CondTraverseOp::expand_batch, ExpandIntoOp, algo.BFS).  It calls the device engine only through
 * include/fgpu.h.  This header flattens it to plain C so that tests (ctypes) and embedders can drive it;
 * every function names the reference method it forwards to (file:line relative to
 * /root/reference/graph/src).  Return value: 0 ok, 1 = GrB_NO_VALUE where noted, negative = fgpu_info;
 * fh_last_error() holds the message.  Out arrays are malloc'ed and released with fh_free().
 */
#ifndef FALKOR_HOST_H
#define FALKOR_HOST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fh_ctx fh_ctx;     /* matrix::init context                         graphblas/matrix.rs:116-221 */
typedef struct fh_mat fh_mat;     /* Matrix<bool> / Matrix<u64>                   graphblas/matrix.rs */
typedef struct fh_vm fh_vm;       /* VersionedMatrix<bool> (Delta_Matrix)         graphblas/versioned_matrix.rs */
typedef struct fh_graph fh_graph; /* traversal-facing slice of Graph              graph/graph.rs */

int fh_init(fh_ctx** ctx, int device);
void fh_finalize(fh_ctx* ctx);
const char* fh_last_error(void);
void fh_free(void* p);

/* fold policy — versioned_matrix.rs:152-200 (pure integer arithmetic; needs no device) */
int fh_should_fold(uint64_t delta_nvals, uint64_t tx_added, uint64_t base_nvals);
int fh_should_fold_read(uint64_t delta_nvals, uint64_t tx_added, uint64_t base_nvals);
int fh_delta_dominates_base(uint64_t delta_nvals, uint64_t base_nvals);
/* tensor.rs:154-163; returns -3 when an id needs more than 32 bits */
int fh_compound_key(uint64_t src, uint64_t dst, uint64_t* key);

/* ---- Matrix<T>: type 0 = bool, 1 = u64 ------------------------------------------------------------ */
int fh_mat_new(fh_ctx* ctx, fh_mat** out, int type, uint64_t nrows, uint64_t ncols);   /* matrix.rs:1151, 1214 */
void fh_mat_free(fh_mat* m);
int fh_mat_build(fh_mat* m, const uint64_t* rows, const uint64_t* cols, const uint64_t* vals, uint64_t n); /* :1186, :1281 */
int fh_mat_set(fh_mat* m, uint64_t i, uint64_t j, uint64_t v);                         /* :1174, :1264 */
int fh_mat_remove(fh_mat* m, uint64_t i, uint64_t j);                                  /* :664 */
int fh_mat_get(fh_mat* m, uint64_t i, uint64_t j, uint64_t* v);                        /* :1158, :1248; 1 = NO_VALUE */
int fh_mat_nvals(fh_mat* m, uint64_t* out);                                            /* :722 */
int fh_mat_dims(fh_mat* m, uint64_t* nrows, uint64_t* ncols);
int fh_mat_pending(fh_mat* m, int* out);                                               /* :764 */
int fh_mat_wait(fh_mat* m);                                                            /* :781 */
/* matrix::Iter as a reusable streaming cursor (matrix.rs:1471-1605): new / seek (re-aim, :1542-1570) / next.
 * fh_mat_cursor_next fills up to `cap` entries of the caller's arrays (vals nullable); *n < cap = exhausted. */
typedef struct fh_mat_cursor fh_mat_cursor;
int fh_mat_cursor_new(fh_mat* m, uint64_t min_row, uint64_t max_row, fh_mat_cursor** out);
int fh_mat_cursor_seek(fh_mat_cursor* c, uint64_t min_row, uint64_t max_row);
int fh_mat_cursor_next(fh_mat_cursor* c, uint64_t cap, uint64_t* rows, uint64_t* cols, uint64_t* vals, uint64_t* n);
void fh_mat_cursor_free(fh_mat_cursor* c);
int fh_mat_iter(fh_mat* m, uint64_t min_row, uint64_t max_row, uint64_t** rows, uint64_t** cols,
                uint64_t** vals, uint64_t* n);                                         /* Iter :1471-1605 */
int fh_mat_dup(fh_mat* m, fh_mat** out);                                               /* :370 */
int fh_mat_transpose(fh_mat* m, fh_mat** out);                                         /* :633 */
int fh_mat_grown(fh_mat* m, uint64_t nrows, uint64_t ncols, fh_mat** out);             /* :664-704 */
int fh_mat_resize(fh_mat* m, uint64_t nrows, uint64_t ncols);                          /* :576 */
int fh_mat_lmxm(fh_mat* self, fh_mat* b);                                              /* :930 */
int fh_mat_rmxm(fh_mat* self, fh_mat* b);                                              /* :951 */
int fh_mat_delta_lmxm(fh_mat* self, fh_mat* m, fh_mat* dp, fh_mat* dm);                /* :1317 */
int fh_mat_intersection_nvals(fh_mat* a, fh_mat* b, uint64_t* out);                    /* :743 */

/* ---- VersionedMatrix<bool> ---------------------------------------------------------------------- */
int fh_vm_new(fh_ctx* ctx, fh_vm** out, uint64_t nrows, uint64_t ncols);               /* versioned_matrix.rs:494 */
int fh_vm_from_coo(fh_ctx* ctx, fh_vm** out, uint64_t nrows, uint64_t ncols, const uint64_t* rows,
                   const uint64_t* cols, uint64_t n);                                  /* from_matrix :877 */
void fh_vm_free(fh_vm* v);
int fh_vm_set(fh_vm* v, uint64_t i, uint64_t j);                                       /* :844 */
int fh_vm_remove(fh_vm* v, uint64_t i, uint64_t j);                                    /* :780 */
int fh_vm_get(fh_vm* v, uint64_t i, uint64_t j);                                       /* :819; 0 present, 1 NO_VALUE */
int fh_vm_nvals(fh_vm* v, uint64_t* out);                                              /* :629 */
int fh_vm_iter(fh_vm* v, uint64_t min_row, uint64_t max_row, uint64_t** rows, uint64_t** cols, uint64_t* n); /* :647 */
int fh_vm_set_all(fh_vm* v, const uint64_t* rows, const uint64_t* cols, uint64_t n, int is_new);   /* :1006 */
int fh_vm_remove_mask(fh_vm* v, const uint64_t* rows, const uint64_t* cols, uint64_t n);           /* :799 */
int fh_vm_dup(fh_vm* v, fh_vm** out);                                                  /* :1038 */
int fh_vm_wait(fh_vm* v);                                                              /* :545 */
int fh_vm_flush(fh_vm* v);                                                             /* :892 */
int fh_vm_fold_oversized(fh_vm* v);                                                    /* :953 */
int fh_vm_extract(fh_vm* v, fh_mat** out);                                             /* :609 */
int fh_vm_transpose(fh_vm* v, fh_vm** out);                                            /* :1070 */
/* out[0..2] = nvals of m, dp, dm; out[3] = needs_flush */
int fh_vm_state(fh_vm* v, uint64_t out[4]);

/* ---- Graph slice ------------------------------------------------------------------------------------ */
int fh_graph_new(fh_ctx* ctx, fh_graph** out, uint64_t node_cap);
void fh_graph_free(fh_graph* g);
int fh_graph_add_label(fh_graph* g, const char* name, uint64_t* id);
int fh_graph_add_type(fh_graph* g, const char* name, uint64_t* id);
int fh_graph_label_node(fh_graph* g, uint64_t node, uint64_t label_id);
int fh_graph_delete_node(fh_graph* g, uint64_t node);
int fh_graph_create_edge(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t edge_id);
int fh_graph_create_edges(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts,
                          const uint64_t* ids, uint64_t n);   /* Tensor::set_all_from_slices + adjacency set_all */
/* The bulk load of one relationship type (the shape of Graph::create_relationships_bulk + flush_for_bulk, graph.rs:2062-2140):
 * one fgpu_edges_build, the result adopted as (or merged into) the tensor's base, the adjacency's base U= its pattern; ends
 * folded.  A batch with a pair that already holds an edge goes through the create_edges path whole.  stats (nullable):
 * [0] edges through the device build, [1] edges through the fallback, [2] distinct pairs, [3] multi-edge pairs, [4] runs that
 * arrived out of id order, [5] of those, sorted by the host.  An invalid batch (a node id at or past the capacity, an id equal
 * to MULTI_EDGE, the same (src, dst, id) twice) returns the engine's code and leaves the graph as it was. */
int fh_graph_bulk_insert_edges(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts,
                               const uint64_t* ids, uint64_t n, uint64_t stats[6]);
/* host-clock phases (ns) of this thread's last fh_graph_bulk_insert_edges (a measurement hook, tools/bench_paths.py load):
 * [0] the fgpu_edges_build call, [1] folding the layers and adopting / merging the built pieces (or the whole fallback),
 * [2] filling the multi-edge map, [3] the adjacency union */
int fh_last_bulk_phases_ns(uint64_t out[4]);
/* CREATE of one relationship type's batch onto a graph that already holds edges (Tensor::set_all_from_slices under
 * Graph::create_relationships_bulk, tensor.rs:333-447, graph.rs:2062-2121, for the whole batch on the device): one
 * fgpu_edges_build, the layers folded, one fgpu_edges_union of the tensor's base with the built batch — a pair that already
 * holds an edge is promoted to MULTI_EDGE or its row extended — the results adopted as the bases, the multi-edge map rewritten
 * for the touched pairs, the adjacency's base U= the batch's pattern; ends folded and never takes the create_edges path.
 * stats (nullable): [0] edges, [1] distinct pairs of the batch, [2] its multi-edge pairs, [3] pairs that collided with a stored
 * one, [4] of those promoted (one edge before), [5] extended (MULTI_EDGE before), [6] rows of the multi-edge map written,
 * [7] runs sorted by the host.  An invalid batch (a node id at or past the capacity, an id equal to MULTI_EDGE, the same
 * (src, dst, id) twice, an id already stored on its pair) returns the engine's code and leaves the graph as it was. */
int fh_graph_append_edges_bulk(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts, const uint64_t* ids,
                               uint64_t n, uint64_t stats[8]);
/* host-clock phases (ns) of this thread's last fh_graph_append_edges_bulk (a measurement hook, tools/bench_paths.py append):
 * [0] the fgpu_edges_build call, [1] the folds, the gather of the multi-edge rows and the fgpu_edges_union call, [2] rewriting
 * the multi-edge map, [3] the adjacency union */
int fh_last_append_phases_ns(uint64_t out[4]);
/* DETACH DELETE of a node set in one call (what Pending::commit does with Graph::delete_nodes + delete_implicit_edges,
 * graph.rs:1698-1772, 2386-2494): every node gets fh_graph_delete_node's effects; per relationship type one fgpu_nodes_detach
 * takes the incident edges out of the tensor, which ends folded; the node x label matrix loses the nodes' rows and the adjacency
 * every entry incident to them (also the pairs with BOTH ends deleted, which the reference leaves behind as unreachable).
 * ids / srcs / dsts (malloc'ed, fh_free; n of each) are the removed edges in the reference's order: types ascending; per type
 * the nodes ascending; per node its out edges by ascending dst, then its in edges from surviving sources by ascending src; the
 * ids of one pair ascending.  The n_skip ids of skip_ids (the reference's explicit_rels; nullable) are left out of the list,
 * but their edges leave the graph like the others: a later fh_graph_delete_edge of one finds the pair absent and does nothing.
 * stats (nullable): [0] distinct nodes, [1] edges removed (the skipped ones included), [2] edges listed, [3] label entries
 * removed, [4] adjacency entries removed, [5] multi-edge pairs removed.  An empty node list does nothing; a node at or past the
 * node capacity returns the engine's code before anything changed. */
int fh_graph_delete_nodes_bulk(fh_graph* g, const uint64_t* nodes, uint64_t n_nodes, const uint64_t* skip_ids, uint64_t n_skip,
                               uint64_t** ids, uint64_t** srcs, uint64_t** dsts, uint64_t* n, uint64_t stats[6]);
/* host-clock phases (ns) of this thread's last fh_graph_delete_nodes_bulk (a measurement hook, tools/bench_paths.py detach):
 * [0] the tensors' fgpu_nodes_detach calls with their folds, [1] expanding and ordering the lists on the host, [2] the label
 * matrix, [3] the adjacency */
int fh_last_detach_phases_ns(uint64_t out[4]);
/* DELETE r of n_edges edges in one call (the shape of Graph::delete_relationships, graph.rs:2268-2373): edge k is (types[k],
 * srcs[k], dsts[k], edge_ids[k]).  The batch is grouped by type; per type, ascending, one fgpu_edges_remove takes the named edges
 * out of the tensor, which ends folded: a single-edge pair leaves, a multi-edge pair shrinks, is demoted to an inline id or
 * leaves.  Every named id leaves the vector indexes of its type; the pairs a tensor emptied and no type still connects leave the
 * adjacency.  A removal applies only where the id is there: an unknown id, an id of another pair and an absent pair change nothing.
 * ids / out_srcs / out_dsts (malloc'ed, fh_free; n of each) are the removed edges: types ascending, input order within a type,
 * a repeated edge once.  stats (nullable): [0] edges named, [1] edges removed, [2] pairs emptied (summed over the types),
 * [3] multi-edge pairs demoted, [4] adjacency entries removed.  per_type (nullable; malloc'ed, n_types entries) = edges removed
 * per type.  An unknown type or a node id at or past the capacity returns the engine's code before anything changed. */
int fh_graph_delete_edges_bulk(fh_graph* g, const uint64_t* types, const uint64_t* srcs, const uint64_t* dsts, const uint64_t* edge_ids,
                               uint64_t n_edges, uint64_t** ids, uint64_t** out_srcs, uint64_t** out_dsts, uint64_t* n,
                               uint64_t stats[5], uint64_t** per_type, uint64_t* n_types);
/* host-clock phases (ns) of this thread's last fh_graph_delete_edges_bulk (a measurement hook, tools/bench_paths.py edel):
 * [0] gathering the multi-edge rows of the touched pairs, [1] the tensors' folds and fgpu_edges_remove calls, [2] rewriting the
 * multi-edge map, [3] the adjacency */
int fh_last_edge_delete_phases_ns(uint64_t out[4]);
int fh_graph_delete_edge(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t edge_id);
/* MVCC commit of every matrix: dup() (fold decision) then fold_oversized, as mvcc_graph.rs:161-180 does */
int fh_graph_commit(fh_graph* g);
int fh_graph_node_has_label(fh_graph* g, uint64_t node, uint64_t label_id);            /* graph.rs:1057; 0 yes, 1 no */
int fh_tensor_get(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t** ids, uint64_t* n); /* tensor.rs:307 */
int fh_tensor_edge_count(fh_graph* g, uint64_t type_id, uint64_t* out);                /* tensor.rs:955 */
int fh_tensor_iter_edges(fh_graph* g, uint64_t type_id, uint64_t** srcs, uint64_t** dsts, uint64_t** ids,
                         uint64_t* n);                                                  /* tensor.rs:973 */
/* out[0..2] = nvals of fwd m, dp, dm; out[3] = multi pairs; out[4] = nvals of mt (effective) */
int fh_tensor_state(fh_graph* g, uint64_t type_id, uint64_t out[5]);

/* A Tensor on its own (tensor.rs:184-989) — what the unit tests of tensor.rs:1340-1669 drive.
 * rels = n triples (edge id, src, dst) as Tensor::remove_all takes them; emptied = the pairs left without an edge.
 * fh_tn_op: 0 flush, 1 fold_oversized, 2 wait (every layer), 3 wait_fwd, 4 resize(a, b).
 * fh_tn_probe: which 0 = effective forward value (eff_get; the MULTI_EDGE sentinel is UINT64_MAX), 1 = committed base
 * m, 2 = extract() pattern; returns 1 (GrB_NO_VALUE) when absent.
 * fh_tn_state: nvals of m, dp, dm; multi pairs; nvals of mt.extract(); ids held in me; edge_count; m.pending(). */
typedef struct fh_tn fh_tn;
int fh_tn_new(fh_ctx* ctx, fh_tn** out, uint64_t nrows, uint64_t ncols);
void fh_tn_free(fh_tn* t);
int fh_tn_dup(fh_tn* t, fh_tn** out);
int fh_tn_set_all(fh_tn* t, const uint64_t* srcs, const uint64_t* dsts, const uint64_t* ids, uint64_t n);
int fh_tn_remove_all(fh_tn* t, const uint64_t* rels, uint64_t n, uint64_t** emptied_src, uint64_t** emptied_dst,
                     uint64_t* n_emptied);
int fh_tn_op(fh_tn* t, int op, uint64_t a, uint64_t b);
int fh_tn_get(fh_tn* t, uint64_t src, uint64_t dst, uint64_t** ids, uint64_t* n);
int fh_tn_probe(fh_tn* t, int which, uint64_t src, uint64_t dst, uint64_t* val);
int fh_tn_state(fh_tn* t, uint64_t out[8]);
/* Encode<19> / Decode<19> for Tensor (tensor.rs:1053-1209): forward matrix (multi-edge pairs as count | 1 << 63), empty
 * dp / dm, edge count, tensor section (base group, delta-plus group) of (src, dst, id-list blob).  The blob of the
 * default codec is this library's plain list; a GxB_Vector_serialize blob needs GraphBLAS (see serialize.cpp). */
int fh_tn_encode(fh_tn* t, uint8_t** bytes, uint64_t* len);
int fh_tn_decode(fh_ctx* ctx, const uint8_t* bytes, uint64_t len, fh_tn** out, uint64_t* consumed);
/* the dup() Graph::new_version takes of one type's tensor (graph.rs:851-890), as a handle of its own (fh_tn_free): the version
 * a reader holds while the graph goes on being written */
int fh_graph_tensor_version(fh_graph* g, uint64_t type_id, fh_tn** out);

/* Raw layer dump for tests: type_id < 0 = the adjacency matrix; which 0 = m, 1 = dp, 2 = dm. */
int fh_graph_layer_iter(fh_graph* g, int64_t type_id, int which, uint64_t** rows, uint64_t** cols,
                        uint64_t** vals, uint64_t* n);

/* ---- operators ---------------------------------------------------------------------------------------
 * `spec` is "key=value;..." with keys: src=<labels,>  hop=<types,>|<dst labels,> (repeatable: hop 0 then the
 * fused chain)  optional= bind= emit= bidir= siblings= attrs= transposed= (0/1).
 * src[i] / to_bound[i]: node id, -1 = unbound, -2 = bound to NULL / a non-node.
 * transposed=1: src[i] is the matrix DESTINATION (cond_traverse.rs:221-235); the batch runs over the transposed layers and
 * out_dest holds the matrix sources reached — row-equal to fh_cond_traverse_rows(..., transposed = 1) (an extension: the
 * reference takes these per row). */
int fh_cond_traverse_batch(fh_graph* g, const char* spec, const int64_t* src, const int64_t* to_bound,
                           uint64_t k, int* batched, uint64_t** out_row, uint64_t** out_dest,
                           int64_t** out_edge, uint64_t* n, uint64_t** null_rows, uint64_t* n_null,
                           uint64_t* flops);                                            /* cond_traverse.rs:452-751 */
/* duration (ns) of the C++ operator inside this thread's last fh_cond_traverse_batch / fh_algo_bfs / fh_algo_pagerank /
 * fh_algo_wcc / fh_algo_betweenness call:
 * what the operator costs without the ctypes harness' result copies (tools/bench_paths.py host) */
uint64_t fh_last_op_ns(void);
int fh_cond_traverse_eligible(const char* spec);                                       /* cond_traverse.rs:308-316 */
int fh_cond_traverse_row(fh_graph* g, const char* spec, int64_t from_id, int64_t to_id, int transposed,
                         uint64_t** out_from, uint64_t** out_to, uint64_t** out_edge, uint64_t* n); /* :758-1117 */
/* The per-row fallback over one input batch of k rows (from / to: node id, -1 unbound, -2 bound to a non-node), with
 * the sibling-edge uniqueness list and, when dedup_src != NULL, the cross-row (scan source, final dest) dedup of an
 * anonymous bidirectional CT over an anonymous bidirectional child (cond_traverse.rs:262-299, 948-970). */
int fh_cond_traverse_rows(fh_graph* g, const char* spec, const int64_t* from_ids, const int64_t* to_ids,
                          const int64_t* dedup_src, uint64_t k, int transposed, const uint64_t* used_edges,
                          uint64_t n_used, uint64_t** out_row, uint64_t** out_from, uint64_t** out_to,
                          uint64_t** out_edge, uint64_t* n);
/* The same input batch on the device (CondTraverseOp::expand_batch_edges over ONE fgpu_expand_edges): the same spec and the same
 * four columns, row-equal to fh_cond_traverse_rows, for a single hop without inline attributes that emits the relationship, is
 * bidirectional or has sibling edge aliases.  *batched = 0, with nothing run and every output empty, when the op declines: a
 * fused chain, a pattern the matrix path serves, or cross_row_dedup != 0 (the caller would pass dedup_src: that case stays per
 * row).  used_edges (nullable): k * n_used ids, row i's sibling-bound ids at used_edges[i * n_used ..], padded with ~0.
 * null_rows: the input rows an OPTIONAL traverse null-pads, those without an emission.  stats (nullable): fgpu_expand_edges'. */
int fh_cond_traverse_edges_batch(fh_graph* g, const char* spec, const int64_t* from_ids, const int64_t* to_ids, uint64_t k,
                                 int transposed, int cross_row_dedup, const uint64_t* used_edges, uint64_t n_used, int* batched,
                                 uint64_t** out_row, uint64_t** out_from, uint64_t** out_to, uint64_t** out_edge, uint64_t* n,
                                 uint64_t** null_rows, uint64_t* n_null, uint64_t stats[8]);
/* SemiApply / AntiSemiApply (semi_apply.rs:85-106) over one argument batch: the pattern predicate `WHERE (a)-[:T]->()`,
 * `WHERE NOT ...`, the anti-join `WHERE NOT (a)-[:T]->(c)`.  spec: the CondTraverse spec above, the right branch.  from_ids /
 * to_ids as fh_cond_traverse_rows takes them (a node id, -1 unbound, -2 Null or not a node: such a row emits nothing, so it does
 * not match); to_ids nullable: no row has it bound.  A row passes iff (the branch emits for it) XOR anti; *passing (fh_free):
 * the passing input rows, ascending.  *tier (nullable): 1 the existence tier answered (fgpu_expand_exists, or the probe when
 * every row has `to` bound: nothing expanded), 2 the collect tier (the pairs expanded and the rows that occur: the reference's
 * method, and all that runs with device_exists == 0), 3 row by row, 0 no row could match.  stats (nullable): fgpu_expand_exists'
 * four summed over the calls made, then the number of calls. */
int fh_semi_apply(fh_graph* g, const char* spec, int anti, int device_exists, const int64_t* from_ids, const int64_t* to_ids,
                  uint64_t k, int transposed, uint64_t** passing, uint64_t* n, int* tier, uint64_t stats[5]);
/* OrApplyMultiplexer (or_apply_multiplexer.rs:85-123): n_branches branches over the same rows; a row passes when any branch
 * passes, branch b inverted when anti[b].  Branch b is the pattern specs[b], or — specs[b] NULL — the caller's boolean column
 * columns[b] (k bytes: a filter branch such as `p.id = 0`).  anti / transposed nullable (all 0); tiers (n_branches) and stats
 * (5 per branch) nullable, per branch as fh_semi_apply reports them. */
int fh_or_apply(fh_graph* g, const char* const* specs, const uint8_t* const* columns, const int* anti, const int* transposed,
                int n_branches, int device_exists, const int64_t* from_ids, const int64_t* to_ids, uint64_t k,
                uint64_t** passing, uint64_t* n, int* tiers, uint64_t* stats);
/* types: comma list ("" = all).  batched != 0 runs the whole input through one set of device probes. */
int fh_expand_into(fh_graph* g, const char* types, int bidirectional, int emit_relationship, int batched,
                   const uint64_t* srcs, const uint64_t* dsts, uint64_t k, uint64_t** out_row,
                   uint64_t** out_src, uint64_t** out_dst, uint64_t** out_edge, uint64_t* n);  /* expand_into.rs:121-258 */
/* CondVarLenTraverse, one input row (cond_var_len_traverse.rs:81-387): the trail DFS of (start)-[:types*min..max]-(far end)
 * in the reference's emission order.  types / dst_labels: comma lists ("" = all / none).  reversed: the bound endpoint is the
 * pattern's `to` (walk incoming edges); max_hops = UINT32_MAX: unbounded; dest < 0: the far end is not bound.  emit_path:
 * `path` holds node, edge, node, ... of every row back to back in pattern order, `path_off` (n + 1 offsets) cuts it.
 * prune != 0: with a bound far end the device computes which nodes can still reach it within the remaining budget and
 * branches outside that set are not expanded (same rows, same order).  stats (nullable): frames expanded, continuations
 * pruned, device products spent on the reach sets. */
int fh_var_len_traverse(fh_graph* g, const char* types, const char* dst_labels, int reversed, int bidirectional,
                        uint32_t min_hops, uint32_t max_hops, uint64_t start, int64_t dest, int emit_path, int prune,
                        uint64_t** out_from, uint64_t** out_to, uint64_t** path, uint64_t** path_off, uint64_t* n,
                        uint64_t stats[3]);
/* The same operator over an input batch of k rows on the device (CondVarLenTraverseOp::expand_batch over fgpu_expand_trails):
 * row i of the result is exactly what fh_var_len_traverse gives for (starts[i], dests[i]), rows ascending, out_row the input row
 * of every emission.  dests: nullable (none bound), else per row a node id or < 0.  A row whose start or dest is at or past the
 * node capacity, or deleted, runs on the host and is spliced in at its place; an unknown destination label gives no rows and no
 * device call.  device_budget: the frames + emissions one device call may hold (0 = the operator's default, 2^22): a batch that
 * does not fit is split in two, a single row that does not fit runs on the host, with `prune` as set.  The device does not prune.
 * stats (nullable): frames (device calls that answered + host rows), pruned and reach products (host rows only).  device_calls
 * (nullable): fgpu_expand_trails calls made, refused ones included. */
int fh_var_len_traverse_batch(fh_graph* g, const char* types, const char* dst_labels, int reversed, int bidirectional,
                              uint32_t min_hops, uint32_t max_hops, const uint64_t* starts, const int64_t* dests, uint64_t k,
                              int emit_path, int prune, uint64_t device_budget, uint64_t** out_row, uint64_t** out_from,
                              uint64_t** out_to, uint64_t** path, uint64_t** path_off, uint64_t* n, uint64_t stats[3],
                              uint64_t* device_calls);
/* AllShortestPathsOp, one input row (all_shortest_paths.rs:82-303): every shortest path of
 * allShortestPaths((src)-[:types*..max_hops]->(dst)), src / dst = the pattern's from / to node, as relationship-id lists in the
 * reference's emission sequence and per-path edge order.  types: a comma list ("" = all); bidirectional: the pattern has no
 * arrow; reversed: it is written right to left (the lists are reversed once more); max_hops = UINT32_MAX: unbounded.
 * src == dst asks for the shortest cycles through src.  The search is one fgpu_shortest_dag call (see fgpu.h); limit > 0 stops
 * the enumeration after that many paths.  *length = the paths' length (-1: none); `edges` holds the paths back to back,
 * `path_off` (n_paths + 1 offsets) cuts it; both are freed with fh_free.  Edge-attribute filters are not served. */
int fh_all_shortest_paths(fh_graph* g, const char* types, int bidirectional, int reversed, uint32_t max_hops, uint64_t src,
                          uint64_t dst, uint64_t limit, int64_t* length, uint64_t** edges, uint64_t** path_off, uint64_t* n_paths);
/* AllShortestPathsOp over a parent batch of `count` input rows, row i = (srcs[i], dsts[i]): lengths[i] and the paths of row i are
 * what fh_all_shortest_paths gives for that row under the same limit (applied per row).  The pattern matrix and its transpose
 * are built once, ONE fgpu_shortest_dag_batch call serves every row whose nodes are in range and alive (a row with an
 * out-of-range or deleted node, and every row when no type resolves, has length -1 and no path and never reaches the device),
 * and the relationship ids come from one tensor probe per type and direction.  `edges` holds all paths back to back,
 * `path_off` (row_off[count] + 1 offsets) cuts it into paths, row_off (count + 1 entries, the caller's) the paths into rows;
 * edges and path_off are freed with fh_free.  *device_calls (nullable) = the fgpu_shortest_dag_batch calls made, 0 or 1. */
int fh_all_shortest_paths_batch(fh_graph* g, const char* types, int bidirectional, int reversed, uint32_t max_hops,
                                const uint64_t* srcs, const uint64_t* dsts, uint64_t count, uint64_t limit, int64_t* lengths,
                                uint64_t** edges, uint64_t** path_off, uint64_t* row_off, uint64_t* device_calls);
/* shortestPath((src)-[:types*min_hops..max_hops]->(dst)) for one row (eval.rs:1301-1513): the ONE path the reference's
 * bidirectional search returns (the rules are in fgpu.h under fgpu_shortest_path_batch), walked on the host through the versioned
 * matrices' iterators.  types: a comma list ("" = none named); directed 0: the pattern has no arrow; min_hops 0 or 1;
 * max_hops = UINT32_MAX: unbounded.  src / dst: a node id, -1 for Null (the path is null), below -1 for a value that is not a
 * node (fails with "A shortestPath requires bound nodes").  *is_null = 1: no path, both lists empty.  Otherwise `nodes` holds
 * the path's node ids (one with min_hops 0 and src == dst) and `edges` the relationship of each consecutive pair (u, v): the
 * first id from u to v over the types in order, else the first from v to u, else none — so n_edges may be below n_nodes - 1.
 * Both are freed with fh_free. */
int fh_shortest_path(fh_graph* g, const char* types, int directed, uint32_t min_hops, uint32_t max_hops, int64_t src, int64_t dst,
                     int* is_null, uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, uint64_t* n_edges);
/* shortestPath() over a parent batch of `count` rows, row i = (srcs[i], dsts[i]): what fh_shortest_path gives for each row.
 * The forward and backward patterns are built once, ONE fgpu_shortest_path_batch call serves every row whose two nodes are in
 * range, alive and different (no row when no type resolves), the relationship ids come from one tensor probe per type and
 * direction, and the other rows are evaluated on the host in place.  is_null, node_off and edge_off are the caller's (count,
 * count + 1 and count + 1 entries): nodes[node_off[i] .. node_off[i + 1]) and edges[edge_off[i] .. edge_off[i + 1]) are row i's.
 * nodes and edges are freed with fh_free.  *device_calls (nullable) = the fgpu_shortest_path_batch calls made, 0 or 1. */
int fh_shortest_path_batch(fh_graph* g, const char* types, int directed, uint32_t min_hops, uint32_t max_hops, const int64_t* srcs,
                           const int64_t* dsts, uint64_t count, uint8_t* is_null, uint64_t** nodes, uint64_t* node_off,
                           uint64_t** edges, uint64_t* edge_off, uint64_t* device_calls);
/* indegree(n [, types]) / outdegree(n [, types]) (entity.rs:268-381, graph.rs:1839-1887) for `k` node ids: out[i] = the number
 * of relationships that enter (incoming != 0) or leave ids[i], the relationships of a multi-edge pair counted one by one, a
 * self-loop once per direction.  types: a comma list; "" = every tensor, a name listed twice counts once, an unknown name is
 * dropped, and when no listed name is known every answer is 0.  mode 0: one row at a time on the host, the count of the
 * reference's iterator loop; mode 1: the layers of the resolved tensors go to ONE fgpu_node_degrees call per 64 of them.
 * Pending creations and deletions (dp / dm) are counted in both modes.  An id at or past the node capacity fails before any
 * result; a deleted node answers 0 once its relationships are gone.  out is the caller's (k entries); *device_calls
 * (nullable) = the fgpu_node_degrees calls made. */
int fh_node_degrees(fh_graph* g, const char* types, int incoming, const uint64_t* ids, uint64_t k, int mode, uint64_t* out,
                    uint64_t* device_calls);
/* The same for every node id below the node capacity, through the whole-graph form of fgpu_node_degrees: (*out)[v], v < *n,
 * with *n the node capacity.  *out is freed with fh_free. */
int fh_node_degrees_all(fh_graph* g, const char* types, int incoming, uint64_t** out, uint64_t* n);
/* source < 0 = NULL; rel_type NULL = all types.  `edges` holds one id per (parent, child) pair that HAS a
 * representative edge among the types, in node order; a pair without one is skipped in `edges` but its child stays in
 * `nodes` — exactly what the reference yields (algo_procedures.rs:1121-1150) — so the two lists are parallel only
 * while n_edges == n_nodes, which holds whenever the adjacency was built from the same types. */
int fh_algo_bfs(fh_graph* g, int64_t source, int64_t max_depth, const char* rel_type, int want_edges,
                int* has_row, uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, uint64_t* n_edges); /* algo_procedures.rs:1021-1160 */

/* The same procedure partitioned over the contexts of `gang` (one per GPU; gang[0] = the graph's context): nnz-balanced
 * column slabs, level loop + frontier exchange inside libfgpu.so (fgpu_bfs_dist_run).  Same output. */
int fh_algo_bfs_multi(fh_graph* g, fh_ctx* const* gang, int n_gang, int64_t source, int64_t max_depth,
                      const char* rel_type, int want_edges, int* has_row, uint64_t** nodes, uint64_t* n_nodes,
                      uint64_t** edges, uint64_t* n_edges);

/* The v19 on-disk form of a Matrix<T> (Encode<19> / Decode<19>, matrix.rs:428-546): the 608 bytes of
 * GxB_Container_struct + its vectors x, h, p, i, b in Vector<bool>'s unload-to-array form (vector.rs:241-309).
 * Stream framing: unsigned / signed = 8 bytes little-endian, buffer = unsigned length + bytes.
 * fh_container_parse is CPU-only: dims = {nrows, ncols, nvals, hypersparse, valued, bytes consumed}; p (np entries),
 * h (nh), i (nvals), x (nvals when valued) are returned as u64 arrays (fh_free). */
int fh_container_parse(const uint8_t* bytes, uint64_t len, uint64_t* dims, uint64_t** p, uint64_t* np, uint64_t** h,
                       uint64_t* nh, uint64_t** i, uint64_t** x);
int fh_mat_decode(fh_ctx* ctx, const uint8_t* bytes, uint64_t len, fh_mat** out, uint64_t* consumed);
int fh_mat_encode(fh_mat* m, uint8_t** bytes, uint64_t* len);   /* the wait()ed state; free with fh_free */

/* build_adjacency_matrix (graph.rs:3870-3894) or, symmetric != 0, build_symmetric_adjacency_matrix (:3898-3907):
 * types = comma-separated relationship types, "" / NULL = the adjacency of all types */
int fh_graph_build_adjacency(fh_graph* g, const char* types, int symmetric, fh_mat** out);

/* fuse_anonymous_traverse (planner/optimizer/fuse_anonymous_traverse.rs:83-284) on a plan in the text form
 * documented in falkordb_amd/host/planner.cpp; *out_text = the plan after the pass, *spec (nullable) = the runtime
 * spec (fh_cond_traverse_batch format) of CondTraverse node `lower_id` of the result.  Free both with fh_free. */
int fh_plan_fuse(const char* plan_text, int lower_id, char** out_text, char** spec);

/* label / rel_type NULL = all; nodes ascending, scores[k] = centrality of nodes[k] (free both with fh_free) */
int fh_algo_pagerank(fh_graph* g, const char* label, const char* rel_type, uint64_t** nodes, double** scores,
                     uint64_t* n);                                                          /* algo_procedures.rs:687-783 */

/* algo.WCC (algo_procedures.rs:789-880; LAGr_ConnectedComponents through lagraph_bindings.rs:521-526 is fgpu_wcc): labels /
 * types = comma lists, "" / NULL = all; several labels select the UNION of their nodes.  Rows in ascending node id, deleted
 * nodes dropped.  component_ids[k] = the smallest node id of nodes[k]'s component — or, with labels, that node's COMPACT
 * index (its rank among the selected nodes in ascending id order), as the reference returns it.  Free both with fh_free. */
int fh_algo_wcc(fh_graph* g, const char* labels, const char* types, uint64_t** nodes, int64_t** component_ids,
                uint64_t* n);

/* algo.labelPropagation (algo_procedures.rs:1168-1270; LAGraph_cdlp through lagraphx_bindings.rs:218-223 is fgpu_cdlp, whose
 * comment in fgpu.h states the rules): labels / types = comma lists, "" / NULL = all; several labels select the UNION of their
 * nodes (an induced subgraph of the undirected view).  max_iterations as the procedure's maxIterations (default 10); <= 0
 * fails with "maxIterations must be a positive integer".  Rows in ascending node id, deleted nodes dropped.
 * community_ids[k] = the label nodes[k] ends with, a node id — or, with labels, that node's COMPACT index (its rank among the
 * selected nodes in ascending id order), as the reference returns it.  Free both with fh_free. */
int fh_algo_cdlp(fh_graph* g, const char* labels, const char* types, int64_t max_iterations, uint64_t** nodes,
                 int64_t** community_ids, uint64_t* n);

/* algo.HarmonicCentrality (algo_procedures.rs:2623-2784; LAGr_HarmonicCentrality is fgpu_harmonic, whose comment in fgpu.h
 * states the rules): labels / types = comma lists, "" / NULL = all; several labels select the UNION of their nodes (an induced
 * subgraph of the directed adjacency; the sketches hash the node ids).  An unknown relationship type fails with "Relationship
 * type '<t>' does not exist"; an empty graph or an empty selection gives no rows.  Rows in ascending node id, deleted nodes
 * dropped.  scores[k] = the HyperBall estimate of the sum over the nodes w that nodes[k] reaches of 1 / d(nodes[k], w);
 * reachable[k] = the estimated number of such w, nodes[k] itself not counted.  Free the three with fh_free. */
int fh_algo_harmonic_centrality(fh_graph* g, const char* labels, const char* types, uint64_t** nodes, double** scores,
                                int64_t** reachable, uint64_t* n);

/* algo.MSF (algo_procedures.rs:1272-1857; LAGraph_msf through lagraphx_bindings.rs:261-267 is fgpu_msf, whose comment in fgpu.h
 * states the edge order): labels / types = comma lists, "" / NULL = all; several labels select the UNION of their nodes.  An
 * unknown relationship type fails with "Relationship type '<t>' does not exist"; an empty graph or an empty selection gives no
 * trees.  maximize != 0 is objective: 'maximize' (scores negated).  The host mirror has no attribute store, so the weight
 * attribute is data: weights[k] is the attribute of relationship edge_ids[k], k < n_weights (an Int attribute widened by the
 * caller).  edge_ids == NULL means no weightAttribute: every score is 1.0.  A relationship that is not listed has no such
 * attribute and scores +inf under either objective.  Every unordered node pair keeps its smallest-score relationship over the
 * selected types' effective edges (pending additions and deletions applied, multi-edges included), ties to the smallest id.
 * Result, CSR-like: n_trees trees in ascending order of their smallest node id; nodes[node_off[t] .. node_off[t + 1]) the
 * tree's nodes ascending; edges[edge_off[t] .. edge_off[t + 1]) the chosen relationship of each of its forest pairs, the
 * pairs in ascending (min, max) order.  An isolated selected node is a tree without edges.  Free the four with fh_free. */
int fh_algo_msf(fh_graph* g, const char* labels, const char* types, int maximize, const uint64_t* edge_ids, const double* weights,
                uint64_t n_weights, uint64_t* n_trees, uint64_t** node_off, uint64_t** nodes, uint64_t** edge_off,
                uint64_t** edges);

/* fh_algo_msf, fh_algo_sp_paths and the pruning table of fh_algo_sp_paths_rows build their weight matrix on the device, with one
 * fgpu_pair_weights over the selected tensors' own layers (fgpu.h).  stats receives the eight stats of the last such call on g:
 * [0] stored entries examined, [1] relationships examined, [2] candidates, [3] pairs out, [4] dropped as non-finite, [5] took the
 * default, [6] multi-edge pairs expanded, [7] most candidates of one pair; all 0 before the first call, after a call that
 * selected no tensor, and after a refused negative weight. */
int fh_graph_pair_stats(fh_graph* g, uint64_t stats[8]);

/* algo.maxFlow (algo_procedures.rs:2786-3248; LAGr_MaxFlow through lagraphx_bindings.rs:610-618 is fgpu_maxflow, whose comment
 * in fgpu.h states what the returned flow satisfies): labels = a comma list, "" / NULL = all nodes, else a relationship counts
 * when both its ends carry one of the labels; types = exactly one relationship type.  sources / targets: the node ids of
 * sourceNodes / targetNodes.  The host mirror has no attribute store, so the capacity attribute is data: caps[k] is the
 * attribute of relationship edge_ids[k], k < n_caps (an Int attribute widened by the caller; a value that is no number is left
 * out); has_attribute = 0 means the graph does not know the attribute name at all.  A relationship whose listed capacity is
 * >= 0 uses it, every other one uses default_capacity when has_default != 0.  Failures, each with a message that holds the
 * quoted phrase: not exactly one type; an unknown type; a type with "multi-edges"; an empty source or target list ("expects at
 * least one source"); overlapping sets ("disjoint"); a relationship without a usable capacity and no default ("invalid or
 * missing attribute"); max >= min * (2^32 - 1) over the positive capacities ("capacity range too wide").
 * The relationships are the type's effective edges (pending additions and deletions applied); capacities <= 0 are dropped
 * before the solve; no surviving relationship gives three empty lists and 0.0.  Node ids are used as they are when there is no
 * label filter and no deleted node, otherwise compacted; several sources (targets) hang under a super-source (-sink) by arcs of
 * 2^31 - 1, which never appear in the result.
 * Result: nodes = the ascending ends of the relationships with non-zero flow; edges / flows = those relationships and their
 * flows in the order the tensor's edge iteration yields the type's edges — Tensor::iter_edges (tensor.rs:920-933) walks the
 * effective forward matrix row-major, and a type without multi-edges has nothing behind it: ascending (source id, target id);
 * *max_flow = the value.  The value is unique, the assignment is one of the maximum flows.  Free the three with fh_free. */
int fh_algo_maxflow(fh_graph* g, const char* labels, const char* types, const uint64_t* sources, uint64_t n_sources,
                    const uint64_t* targets, uint64_t n_targets, int has_attribute, const uint64_t* edge_ids, const double* caps,
                    uint64_t n_caps, int has_default, double default_capacity, uint64_t** nodes, uint64_t* n_nodes,
                    uint64_t** edges, double** flows, uint64_t* n_edges, double* max_flow);

/* algo.SPpaths (algo_procedures.rs:2548-2597), the branch that answers ONE cheapest path: pathCount 1, no maxLen, no maxCost,
 * source != target — run_path_algo's call of dijkstra_single_path (:2563-2571), computed by fgpu_sssp, whose comment in fgpu.h
 * states which distance and which parent come back.  The other shapes of algo.SPpaths and all of algo.SSpaths enumerate simple
 * paths on the host: fh_algo_sp_paths_rows and fh_algo_ss_paths below.  types = a comma list, "" / NULL = every type; unknown names are dropped, a name listed
 * twice counts once.  direction: 0 outgoing, 1 incoming, 2 both (relDirection).  The host mirror has no attribute store, so
 * weightProp and costProp are data: w_vals[k] is the weight of relationship w_edge_ids[k], k < n_w; w_edge_ids == NULL means no
 * weightProp; a relationship that is not listed weighs 1.0.  c_edge_ids / c_vals / n_c likewise for the cost, default 0.0.  A
 * relationship whose weight is NaN or infinite is left out; a negative weight fails with a message that names the relationship
 * ("negative weight"; the reference leaves the result undefined).  Self-loops are dropped.  Among the relationships that join
 * an ordered pair of nodes in traversal direction the cheapest is used, ties to the smallest id.
 * *found = 0 (and empty lists) when source == target, when either node is deleted or out of range, and when no path exists.
 * Otherwise nodes[0 .. n_nodes) is the path from source to target, edges[0 .. n_nodes - 1) the relationship of every step,
 * *weight the sum of their weights added source -> target in FP64, *cost their costs folded in the same order.  Free the two
 * lists with fh_free. */
int fh_algo_sp_paths(fh_graph* g, uint64_t source, uint64_t target, const char* types, int direction, const uint64_t* w_edge_ids,
                     const double* w_vals, uint64_t n_w, const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, int* found,
                     uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, double* weight, double* cost);

/* algo.SPpaths in EVERY shape (run_path_algo, algo_procedures.rs:2548-2597): pathCount 1 without maxLen and maxCost, source !=
 * target, is fh_algo_sp_paths; every other shape mirrors enumerate_paths + record_found_path + the final sort by
 * cmp_found_path (:2350-2514) and returns the reference's rows in the reference's order.  types, direction and the weight /
 * cost lists as fh_algo_sp_paths takes them, except that a type name listed twice contributes its relationships twice (as
 * get_node_relationships_by_type does).  max_len < 0 = no maxLen; has_max_cost = 0 = no maxCost; path_count: 1 the cheapest
 * path, 0 every path of minimum weight, k > 1 the k cheapest; a negative one fails with "pathCount must be a non-negative
 * integer", a negative weight among the selected relationships with "negative weight".  prune != 0 (the default of the C++
 * layer): the walk skips the successors that cannot end at the target within maxLen, or only above the current weight bound,
 * as decided by the hop-bounded table fgpu_sssp_hops computes from the target over the reversed min-weight matrix (maxLen <=
 * 32 and a table of at most 1 GiB; otherwise by fgpu_sssp's one row, which knows no hop budget: it prunes, but seeds the bound
 * only when maxLen >= n - 1) — host.hpp has the rule and the argument why the rows do
 * not change.  max_examined: a budget of successors taken off the walk's stacks, 0 = none; once spent the call fails
 * ("budget"), which stands for the reference's timeout poll.
 * Result: *n_rows rows; row r has the relationships edges[offsets[r] .. offsets[r + 1]) and the nodes nodes[offsets[r] + r ..
 * offsets[r + 1] + r + 1), weights[r] and costs[r] folded source -> target in FP64.  stats (nullable): [0] successors
 * examined, [1] skipped because the target is out of reach within maxLen, [2] skipped because every completion is above the
 * bound, [3] rows of the table used: -1 none, 0 = fgpu_sssp's one row.  A source or target that is deleted or out of range
 * gives no rows.  Free the five arrays with fh_free. */
int fh_algo_sp_paths_rows(fh_graph* g, uint64_t source, uint64_t target, const char* types, int direction, int64_t max_len,
                          int has_max_cost, double max_cost, int64_t path_count, const uint64_t* w_edge_ids, const double* w_vals,
                          uint64_t n_w, const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, int prune,
                          uint64_t max_examined, uint64_t* n_rows, uint64_t** offsets, uint64_t** nodes, uint64_t** edges,
                          double** weights, double** costs, int64_t stats[4]);
/* algo.SSpaths: the same walk without a target — every non-empty simple path from source qualifies (within maxLen / maxCost),
 * kept and ordered by the same rules.  No device call is made: there is nothing to bound against (stats[3] = -1). */
int fh_algo_ss_paths(fh_graph* g, uint64_t source, const char* types, int direction, int64_t max_len, int has_max_cost,
                     double max_cost, int64_t path_count, const uint64_t* w_edge_ids, const double* w_vals, uint64_t n_w,
                     const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, uint64_t max_examined, uint64_t* n_rows,
                     uint64_t** offsets, uint64_t** nodes, uint64_t** edges, double** weights, double** costs, int64_t stats[4]);

/* algo.betweenness (algo_procedures.rs:884-1017; LAGr_Betweenness through lagraph_bindings.rs:539-546 is fgpu_betweenness):
 * labels / types = comma lists, "" / NULL = all; several labels select the UNION of their nodes (an induced subgraph).
 * sampling_size / sampling_seed as the procedure's samplingSize / samplingSeed (defaults 16 / 0; fh_betweenness_sources).
 * Rows in ascending node id, deleted nodes dropped; scores[k] = the unnormalised centrality of nodes[k].  samplingSize <= 0
 * fails with "samplingSize must be a positive integer".  Free both with fh_free. */
int fh_algo_betweenness(fh_graph* g, const char* labels, const char* types, int64_t sampling_size, int64_t sampling_seed,
                        uint64_t** nodes, double** scores, uint64_t* n);
/* the procedure's source rule alone (algo_procedures.rs:898-975, no GPU): the source indices out of 0..n_nodes, in the order
 * LAGr_Betweenness receives them.  Free *out with fh_free. */
int fh_betweenness_sources(uint64_t n_nodes, int64_t sampling_size, int64_t sampling_seed, uint64_t** out, uint64_t* n);

/* Vector indexes and db.idx.vector.queryNodes / queryRelationships (runtime/ops/node_by_vector_scan.rs,
 * edge_by_vector_scan.rs; Graph::vector_query_nodes / _edges, graph.rs:3408-3520).  An index is an fgpu_vecidx, whose comment
 * in fgpu.h states the rules: the search is exhaustive, rows come in ascending (distance, id).  Node indexes are keyed by
 * (label id, attribute), relationship indexes by (type id, attribute).  The attribute store is out of scope, so the caller
 * feeds the vectors in, as the reference's indexer is fed by property writes.
 * similarity = "euclidean", "cosine", "ip" or NULL (euclidean); anything else fails with "Unknown similarity function
 * '{other}', expected 'euclidean', 'ip', or 'cosine'" (index/mod.rs:1259-1270).  create fails on an (owner, attribute) that
 * is indexed already; drop returns 0 when there was an index, 1 when not. */
int fh_graph_vector_index_create(fh_graph* g, int is_edge, uint64_t label_or_type_id, const char* attr, uint64_t dim,
                                 const char* similarity);
int fh_graph_vector_index_drop(fh_graph* g, int is_edge, uint64_t label_or_type_id, const char* attr);
/* Upsert one entity's vector of n components.  No index on (label / type, attr) fails; n other than the index's dimension
 * fails with "Vector dimension mismatch, expected {dim} but got {n}"; a NaN or infinite component fails.  A relationship index
 * keeps (src, dst) per relationship id.  unset returns 0 when the entity had a vector, 1 when not.  fh_graph_delete_node and
 * fh_graph_delete_edge drop the entity's vectors from every index that holds them (test_vecsim.py test09). */
int fh_graph_vector_set_node(fh_graph* g, uint64_t label_id, const char* attr, uint64_t node, const float* vec, uint64_t n);
int fh_graph_vector_set_edge(fh_graph* g, uint64_t type_id, const char* attr, uint64_t src, uint64_t dst, uint64_t edge_id,
                             const float* vec, uint64_t n);
int fh_graph_vector_unset_node(fh_graph* g, uint64_t label_id, const char* attr, uint64_t node);
int fh_graph_vector_unset_edge(fh_graph* g, uint64_t type_id, const char* attr, uint64_t edge_id);
/* CALL db.idx.vector.queryNodes(label, attr, k, q) YIELD node, score: the min(k, indexed) nearest entities, ascending.  k <= 0
 * fails with "Invalid arguments for procedure 'db.idx.vector.queryNodes'" (queryRelationships' for the edge call); qn other
 * than the index's dimension fails with "Vector dimension mismatch, expected {dim} but got {qn}"; an unknown label / type, or
 * no index on (it, attr), gives no rows and is no error (indexer.rs:525-536).  Free the arrays with fh_free. */
int fh_vector_query_nodes(fh_graph* g, const char* label, const char* attr, int64_t k, const float* q, uint64_t qn,
                          uint64_t** ids, double** dist, uint64_t* n);
int fh_vector_query_edges(fh_graph* g, const char* type, const char* attr, int64_t k, const float* q, uint64_t qn,
                          uint64_t** ids, double** dist, uint64_t** srcs, uint64_t** dsts, uint64_t* n);
/* What NodeByVectorScanOp::next does for a whole parent batch (<= 1024 rows, batch.rs) in ONE fgpu_vecidx_knn call: queries =
 * nq rows of qn components.  The rows of query i are ids / dist [offsets[i] .. offsets[i + 1]); offsets has nq + 1 entries. */
int fh_vector_query_nodes_batch(fh_graph* g, const char* label, const char* attr, int64_t k, const float* queries, uint64_t qn,
                                uint64_t nq, uint64_t** offsets, uint64_t** ids, double** dist);
/* vec.euclideanDistance / vec.cosineDistance (spatial.rs:151-203, runtime/vec_distance.rs) on the host in FP64, the D of
 * fgpu_vecidx_knn: metric = "euclidean", "cosine" or "ip".  na != nb fails with "Vector dimension mismatch, expected {na} but
 * got {nb}". */
int fh_vec_distance(const char* metric, const float* a, uint64_t na, const float* b, uint64_t nb, double* out);

#ifdef __cplusplus
}
#endif
#endif /* FALKOR_HOST_H */
