// capi.cpp — C surface of the host layer (include/falkor_host.h): handles, error codes, array hand-off.
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <sstream>

#include "../../include/falkor_host.h"
#include "host.hpp"

using namespace falkor;

struct fh_ctx { Context c; explicit fh_ctx(int d) : c(d) {} };
struct fh_mat { Matrix m; };
struct fh_vm { VersionedMatrix v; };
struct fh_graph { Graph g; fh_graph(Context& c, u64 n) : g(c, n) {} };
struct fh_tn { Tensor t; };

static thread_local std::string g_err;

template <class F>
static int guard(F f) {
    try {
        return f();
    } catch (const GrbError& e) {
        g_err = e.what();
        return e.info ? (int)e.info : -1;
    } catch (const std::exception& e) {
        g_err = e.what();
        return FGPU_INVALID;
    }
}

// a malloc'ed copy of v for the caller to fh_free (never NULL for an empty v)
template <class T>
static T* hand(const std::vector<T>& v) {
    T* p = (T*)malloc((v.size() ? v.size() : 1) * sizeof(T));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    std::string cur;
    std::istringstream in(s);
    while (std::getline(in, cur, sep))
        if (!cur.empty()) out.push_back(cur);
    return out;
}

// a comma list argument ("" or NULL = none; empty items are dropped)
static std::vector<std::string> csv(const char* s) { return split(s ? s : "", ','); }

static thread_local uint64_t g_last_op_ns = 0;   // duration of the last timed operator inside this thread (fh_last_op_ns)

// runs op() as this thread's timed operator.  The interval is op() alone: arguments are unpacked before it unless op does
// that itself, results are copied out after it; an op() that throws leaves the previous duration in place.
template <class F>
static auto timed(F op) {
    const auto t0 = std::chrono::steady_clock::now();
    auto r = op();
    g_last_op_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    return r;
}

static CondTraverseOp parse_spec(const char* spec) {
    CondTraverseOp op;
    for (auto& kv : split(spec ? spec : "", ';')) {
        auto eq = kv.find('=');
        if (eq == std::string::npos) continue;
        std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        if (k == "src") op.src_labels = split(v, ',');
        else if (k == "hop") {
            Hop h;
            auto bar = v.find('|');
            h.types = split(v.substr(0, bar), ',');
            if (bar != std::string::npos) h.dst_labels = split(v.substr(bar + 1), ',');
            op.hops.push_back(h);
        } else if (k == "optional") op.optional = v == "1";
        else if (k == "bind") op.bind_relationship = v == "1";
        else if (k == "emit") op.emit_relationship = v == "1";
        else if (k == "bidir") op.bidirectional = v == "1";
        else if (k == "siblings") op.has_sibling_edges = v == "1";
        else if (k == "attrs") op.has_inline_attrs = v == "1";
        else if (k == "transposed") op.transposed = v == "1";
    }
    if (op.hops.empty()) op.hops.push_back(Hop{});
    return op;
}

extern "C" {

const char* fh_last_error(void) { return g_err.c_str(); }
void fh_free(void* p) { free(p); }

int fh_init(fh_ctx** ctx, int device) {
    return guard([&] { *ctx = new fh_ctx(device); return 0; });
}
void fh_finalize(fh_ctx* ctx) { delete ctx; }

int fh_should_fold(uint64_t d, uint64_t tx, uint64_t base) { return should_fold(d, tx, base) ? 1 : 0; }
int fh_should_fold_read(uint64_t d, uint64_t tx, uint64_t base) { return should_fold_read(d, tx, base) ? 1 : 0; }
int fh_delta_dominates_base(uint64_t d, uint64_t base) { return delta_dominates_base(d, base) ? 1 : 0; }
int fh_compound_key(uint64_t src, uint64_t dst, uint64_t* key) {
    return guard([&] { *key = compound_key(src, dst); return 0; });
}

// ---- Matrix ----------------------------------------------------------------------------------------
int fh_mat_new(fh_ctx* ctx, fh_mat** out, int type, uint64_t nrows, uint64_t ncols) {
    return guard([&] { *out = new fh_mat{Matrix(ctx->c, type ? Type::UInt64 : Type::Bool, nrows, ncols)}; return 0; });
}
void fh_mat_free(fh_mat* m) { delete m; }
int fh_mat_build(fh_mat* m, const uint64_t* rows, const uint64_t* cols, const uint64_t* vals, uint64_t n) {
    return guard([&] {
        std::vector<u64> r(rows, rows + n), c(cols, cols + n), v;
        if (vals) v.assign(vals, vals + n);
        m->m.build(r, c, vals ? &v : nullptr);
        return 0;
    });
}
int fh_mat_set(fh_mat* m, uint64_t i, uint64_t j, uint64_t v) { return guard([&] { m->m.set_element(i, j, v); return 0; }); }
int fh_mat_remove(fh_mat* m, uint64_t i, uint64_t j) { return guard([&] { m->m.remove_element(i, j); return 0; }); }
int fh_mat_get(fh_mat* m, uint64_t i, uint64_t j, uint64_t* v) {
    return guard([&] {
        auto x = m->m.get(i, j);
        if (!x) return 1;
        if (v) *v = *x;
        return 0;
    });
}
int fh_mat_nvals(fh_mat* m, uint64_t* out) { return guard([&] { *out = m->m.nvals(); return 0; }); }
int fh_mat_dims(fh_mat* m, uint64_t* nrows, uint64_t* ncols) {
    *nrows = m->m.nrows();
    *ncols = m->m.ncols();
    return 0;
}
int fh_mat_pending(fh_mat* m, int* out) { *out = m->m.pending() ? 1 : 0; return 0; }
int fh_mat_wait(fh_mat* m) { return guard([&] { m->m.wait(); return 0; }); }
int fh_mat_iter(fh_mat* m, uint64_t min_row, uint64_t max_row, uint64_t** rows, uint64_t** cols, uint64_t** vals,
                uint64_t* n) {
    return guard([&] {
        auto es = m->m.iter(min_row, max_row);
        std::vector<u64> r, c, v;
        for (auto& e : es) { r.push_back(e.row); c.push_back(e.col); v.push_back(e.val); }
        *rows = hand(r);
        *cols = hand(c);
        if (vals) *vals = hand(v);
        *n = es.size();
        return 0;
    });
}
// streaming cursor (matrix::Iter): new / seek / next-batch / free
struct fh_mat_cursor { MatrixIter it; };
int fh_mat_cursor_new(fh_mat* m, uint64_t min_row, uint64_t max_row, fh_mat_cursor** out) {
    return guard([&] { *out = new fh_mat_cursor{MatrixIter(m->m, min_row, max_row)}; return 0; });
}
int fh_mat_cursor_seek(fh_mat_cursor* c, uint64_t min_row, uint64_t max_row) {
    return guard([&] { c->it.seek(min_row, max_row); return 0; });
}
// up to `cap` entries into caller arrays; *n < cap means the cursor is exhausted
int fh_mat_cursor_next(fh_mat_cursor* c, uint64_t cap, uint64_t* rows, uint64_t* cols, uint64_t* vals, uint64_t* n) {
    return guard([&] {
        uint64_t k = 0;
        for (; k < cap; ++k) {
            auto e = c->it.next();
            if (!e) break;
            rows[k] = e->row;
            cols[k] = e->col;
            if (vals) vals[k] = e->val;
        }
        *n = k;
        return 0;
    });
}
void fh_mat_cursor_free(fh_mat_cursor* c) { delete c; }

int fh_mat_dup(fh_mat* m, fh_mat** out) { return guard([&] { *out = new fh_mat{m->m.dup()}; return 0; }); }
int fh_mat_transpose(fh_mat* m, fh_mat** out) { return guard([&] { *out = new fh_mat{m->m.transpose()}; return 0; }); }
int fh_mat_grown(fh_mat* m, uint64_t nrows, uint64_t ncols, fh_mat** out) {
    return guard([&] { *out = new fh_mat{m->m.grown(nrows, ncols)}; return 0; });
}
int fh_mat_resize(fh_mat* m, uint64_t nrows, uint64_t ncols) { return guard([&] { m->m.resize(nrows, ncols); return 0; }); }
int fh_mat_lmxm(fh_mat* self, fh_mat* b) { return guard([&] { self->m.lmxm(b->m); return 0; }); }
int fh_mat_rmxm(fh_mat* self, fh_mat* b) { return guard([&] { self->m.rmxm(b->m); return 0; }); }
int fh_mat_delta_lmxm(fh_mat* self, fh_mat* m, fh_mat* dp, fh_mat* dm) {
    return guard([&] { self->m.delta_lmxm(m->m, dp->m, dm->m); return 0; });
}
int fh_mat_intersection_nvals(fh_mat* a, fh_mat* b, uint64_t* out) {
    return guard([&] { *out = a->m.intersection_nvals(b->m); return 0; });
}

// ---- VersionedMatrix ------------------------------------------------------------------------------------
int fh_vm_new(fh_ctx* ctx, fh_vm** out, uint64_t nrows, uint64_t ncols) {
    return guard([&] { *out = new fh_vm{VersionedMatrix(ctx->c, nrows, ncols)}; return 0; });
}
int fh_vm_from_coo(fh_ctx* ctx, fh_vm** out, uint64_t nrows, uint64_t ncols, const uint64_t* rows,
                   const uint64_t* cols, uint64_t n) {
    return guard([&] {
        Matrix m(ctx->c, Type::Bool, nrows, ncols);
        m.build(std::vector<u64>(rows, rows + n), std::vector<u64>(cols, cols + n));
        *out = new fh_vm{VersionedMatrix::from_matrix(m)};
        return 0;
    });
}
void fh_vm_free(fh_vm* v) { delete v; }
int fh_vm_set(fh_vm* v, uint64_t i, uint64_t j) { return guard([&] { v->v.set(i, j, true); return 0; }); }
int fh_vm_remove(fh_vm* v, uint64_t i, uint64_t j) { return guard([&] { v->v.remove(i, j); return 0; }); }
int fh_vm_get(fh_vm* v, uint64_t i, uint64_t j) { return guard([&] { return v->v.get(i, j) ? 0 : 1; }); }
int fh_vm_nvals(fh_vm* v, uint64_t* out) { return guard([&] { *out = v->v.nvals(); return 0; }); }
int fh_vm_iter(fh_vm* v, uint64_t min_row, uint64_t max_row, uint64_t** rows, uint64_t** cols, uint64_t* n) {
    return guard([&] {
        auto es = v->v.iter(min_row, max_row);
        std::vector<u64> r, c;
        for (auto& e : es) { r.push_back(e.row); c.push_back(e.col); }
        *rows = hand(r);
        *cols = hand(c);
        *n = es.size();
        return 0;
    });
}
int fh_vm_set_all(fh_vm* v, const uint64_t* rows, const uint64_t* cols, uint64_t n, int is_new) {
    return guard([&] {
        std::vector<std::pair<u64, u64>> e(n);
        for (u64 k = 0; k < n; ++k) e[k] = {rows[k], cols[k]};
        v->v.set_all(e, is_new != 0);
        return 0;
    });
}
int fh_vm_remove_mask(fh_vm* v, const uint64_t* rows, const uint64_t* cols, uint64_t n) {
    return guard([&] {
        Matrix mask(v->v.m().ctx(), Type::Bool, v->v.nrows(), v->v.ncols());
        mask.build(std::vector<u64>(rows, rows + n), std::vector<u64>(cols, cols + n));
        v->v.remove_mask(mask);
        return 0;
    });
}
int fh_vm_dup(fh_vm* v, fh_vm** out) { return guard([&] { *out = new fh_vm{v->v.dup()}; return 0; }); }
int fh_vm_wait(fh_vm* v) { return guard([&] { v->v.wait(); return 0; }); }
int fh_vm_flush(fh_vm* v) { return guard([&] { v->v.flush(); return 0; }); }
int fh_vm_fold_oversized(fh_vm* v) { return guard([&] { v->v.fold_oversized(); return 0; }); }
int fh_vm_extract(fh_vm* v, fh_mat** out) { return guard([&] { *out = new fh_mat{v->v.extract()}; return 0; }); }
int fh_vm_transpose(fh_vm* v, fh_vm** out) { return guard([&] { *out = new fh_vm{v->v.transpose()}; return 0; }); }
int fh_vm_state(fh_vm* v, uint64_t out[4]) {
    return guard([&] {
        out[0] = v->v.m().nvals();
        out[1] = v->v.dp().nvals();
        out[2] = v->v.dm().nvals();
        out[3] = v->v.needs_flush() ? 1 : 0;
        return 0;
    });
}

// ---- Graph ------------------------------------------------------------------------------------------------
int fh_graph_new(fh_ctx* ctx, fh_graph** out, uint64_t node_cap) {
    return guard([&] { *out = new fh_graph(ctx->c, node_cap); return 0; });
}
void fh_graph_free(fh_graph* g) { delete g; }
int fh_graph_add_label(fh_graph* g, const char* name, uint64_t* id) { return guard([&] { *id = g->g.add_label(name); return 0; }); }
int fh_graph_add_type(fh_graph* g, const char* name, uint64_t* id) { return guard([&] { *id = g->g.add_type(name); return 0; }); }
int fh_graph_label_node(fh_graph* g, uint64_t node, uint64_t label_id) { return guard([&] { g->g.label_node(node, label_id); return 0; }); }
int fh_graph_delete_node(fh_graph* g, uint64_t node) { return guard([&] { g->g.delete_node(node); return 0; }); }
int fh_graph_create_edge(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t edge_id) {
    return guard([&] { g->g.create_edge(type_id, src, dst, edge_id); return 0; });
}
int fh_graph_create_edges(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts,
                          const uint64_t* ids, uint64_t n) {
    return guard([&] {
        g->g.create_edges(type_id, std::vector<u64>(srcs, srcs + n), std::vector<u64>(dsts, dsts + n),
                          std::vector<u64>(ids, ids + n));
        return 0;
    });
}
int fh_graph_delete_edge(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t edge_id) {
    return guard([&] { g->g.delete_edge(type_id, src, dst, edge_id); return 0; });
}
int fh_graph_commit(fh_graph* g) {
    return guard([&] {
        g->g.fold_oversized_deltas();
        g->g.new_version();
        return 0;
    });
}
int fh_graph_node_has_label(fh_graph* g, uint64_t node, uint64_t label_id) {
    return guard([&] { return g->g.node_has_label_id(node, label_id) ? 0 : 1; });
}
int fh_tensor_get(fh_graph* g, uint64_t type_id, uint64_t src, uint64_t dst, uint64_t** ids, uint64_t* n) {
    return guard([&] {
        auto v = g->g.relationship_tensors().at(type_id).get(src, dst);
        *ids = hand(v);
        *n = v.size();
        return 0;
    });
}

static thread_local uint64_t g_last_bulk_ns[4] = {0, 0, 0, 0};   // phases of this thread's last bulk insert (fh_last_bulk_phases_ns)
int fh_last_bulk_phases_ns(uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = g_last_bulk_ns[k];
    return 0;
}
int fh_graph_bulk_insert_edges(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts,
                               const uint64_t* ids, uint64_t n, uint64_t stats[6]) {
    return guard([&] {
        BulkStats bs = g->g.bulk_insert_edges(type_id, srcs, dsts, ids, n);
        for (int k = 0; k < 4; ++k) g_last_bulk_ns[k] = bs.phase_ns[k];
        if (stats) {
            stats[0] = bs.device_edges; stats[1] = bs.fallback_edges; stats[2] = bs.distinct_pairs;
            stats[3] = bs.multi_pairs; stats[4] = bs.unsorted_runs; stats[5] = bs.host_sorted_runs;
        }
        return 0;
    });
}

static thread_local uint64_t g_last_append_ns[4] = {0, 0, 0, 0};   // phases of this thread's last bulk append
int fh_last_append_phases_ns(uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = g_last_append_ns[k];
    return 0;
}
int fh_graph_append_edges_bulk(fh_graph* g, uint64_t type_id, const uint64_t* srcs, const uint64_t* dsts, const uint64_t* ids,
                               uint64_t n, uint64_t stats[8]) {
    return guard([&] {
        AppendStats as = g->g.append_edges_bulk(type_id, srcs, dsts, ids, n);
        for (int k = 0; k < 4; ++k) g_last_append_ns[k] = as.phase_ns[k];
        if (stats) {
            stats[0] = as.edges; stats[1] = as.distinct_pairs; stats[2] = as.multi_pairs; stats[3] = as.colliding;
            stats[4] = as.promoted; stats[5] = as.extended; stats[6] = as.me_rows; stats[7] = as.host_sorted_runs;
        }
        return 0;
    });
}

static thread_local uint64_t g_last_detach_ns[4] = {0, 0, 0, 0};   // phases of this thread's last bulk node delete
int fh_last_detach_phases_ns(uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = g_last_detach_ns[k];
    return 0;
}
int fh_graph_delete_nodes_bulk(fh_graph* g, const uint64_t* nodes, uint64_t n_nodes, const uint64_t* skip_ids, uint64_t n_skip,
                               uint64_t** ids, uint64_t** srcs, uint64_t** dsts, uint64_t* n, uint64_t stats[6]) {
    return guard([&] {
        DetachStats ds;
        auto rels = g->g.delete_nodes_bulk(std::vector<u64>(nodes, nodes + n_nodes),
                                           skip_ids ? std::vector<u64>(skip_ids, skip_ids + n_skip) : std::vector<u64>(), &ds);
        for (int k = 0; k < 4; ++k) g_last_detach_ns[k] = ds.phase_ns[k];
        std::vector<u64> i(rels.size()), s(rels.size()), d(rels.size());
        for (size_t k = 0; k < rels.size(); ++k) { i[k] = rels[k][0]; s[k] = rels[k][1]; d[k] = rels[k][2]; }
        *ids = hand(i);
        *srcs = hand(s);
        *dsts = hand(d);
        *n = rels.size();
        if (stats) {
            stats[0] = ds.nodes; stats[1] = ds.edges_removed; stats[2] = ds.edges_listed;
            stats[3] = ds.label_entries; stats[4] = ds.adjacency_entries; stats[5] = ds.multi_pairs;
        }
        return 0;
    });
}
static thread_local uint64_t g_last_edge_delete_ns[4] = {0, 0, 0, 0};   // phases of this thread's last bulk edge delete
int fh_last_edge_delete_phases_ns(uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = g_last_edge_delete_ns[k];
    return 0;
}
int fh_graph_delete_edges_bulk(fh_graph* g, const uint64_t* types, const uint64_t* srcs, const uint64_t* dsts, const uint64_t* edge_ids,
                               uint64_t n_edges, uint64_t** ids, uint64_t** out_srcs, uint64_t** out_dsts, uint64_t* n,
                               uint64_t stats[5], uint64_t** per_type, uint64_t* n_types) {
    return guard([&] {
        EdgeDeleteStats es;
        auto rels = g->g.delete_edges_bulk(types, srcs, dsts, edge_ids, n_edges, &es);
        for (int k = 0; k < 4; ++k) g_last_edge_delete_ns[k] = es.phase_ns[k];
        std::vector<u64> i(rels.size()), s(rels.size()), d(rels.size());
        for (size_t k = 0; k < rels.size(); ++k) { i[k] = rels[k][0]; s[k] = rels[k][1]; d[k] = rels[k][2]; }
        *ids = hand(i);
        *out_srcs = hand(s);
        *out_dsts = hand(d);
        *n = rels.size();
        if (stats) {
            stats[0] = es.edges_named; stats[1] = es.edges_removed; stats[2] = es.pairs_emptied;
            stats[3] = es.pairs_demoted; stats[4] = es.adjacency_entries;
        }
        if (per_type) {
            *per_type = hand(es.per_type);
            *n_types = es.per_type.size();
        }
        return 0;
    });
}
int fh_tensor_edge_count(fh_graph* g, uint64_t type_id, uint64_t* out) {
    return guard([&] { *out = g->g.relationship_tensors().at(type_id).edge_count(); return 0; });
}
int fh_tensor_iter_edges(fh_graph* g, uint64_t type_id, uint64_t** srcs, uint64_t** dsts, uint64_t** ids, uint64_t* n) {
    return guard([&] {
        auto es = g->g.relationship_tensors().at(type_id).iter_edges();
        std::vector<u64> s, d, i;
        for (auto& e : es) { s.push_back(e.row); d.push_back(e.col); i.push_back(e.val); }
        *srcs = hand(s);
        *dsts = hand(d);
        *ids = hand(i);
        *n = es.size();
        return 0;
    });
}
int fh_tensor_state(fh_graph* g, uint64_t type_id, uint64_t out[5]) {
    return guard([&] {
        const Tensor& t = g->g.relationship_tensors().at(type_id);
        t.wait_fwd();
        out[0] = t.fwd_m().nvals();
        out[1] = t.fwd_dp().nvals();
        out[2] = t.fwd_dm().nvals();
        out[3] = t.multi_pairs();
        out[4] = t.matrix_t().nvals();
        return 0;
    });
}

// ---- a Tensor on its own (the unit tests of tensor.rs:1340-1669 drive one directly) ----------------------------
int fh_tn_new(fh_ctx* ctx, fh_tn** out, uint64_t nrows, uint64_t ncols) {
    return guard([&] { *out = new fh_tn{Tensor(ctx->c, nrows, ncols)}; return 0; });
}
void fh_tn_free(fh_tn* t) { delete t; }
int fh_tn_dup(fh_tn* t, fh_tn** out) {
    return guard([&] { *out = new fh_tn{t->t.dup()}; return 0; });
}
int fh_graph_tensor_version(fh_graph* g, uint64_t type_id, fh_tn** out) {
    return guard([&] { *out = new fh_tn{g->g.relationship_tensors().at(type_id).dup()}; return 0; });
}
int fh_tn_set_all(fh_tn* t,const uint64_t* srcs, const uint64_t* dsts, const uint64_t* ids, uint64_t n) {
    return guard([&] {
        t->t.set_all_from_slices(std::vector<u64>(srcs, srcs + n), std::vector<u64>(dsts, dsts + n),
                                 std::vector<u64>(ids, ids + n));
        return 0;
    });
}
int fh_tn_remove_all(fh_tn* t, const uint64_t* rels, uint64_t n, uint64_t** emptied_src, uint64_t** emptied_dst,
                     uint64_t* n_emptied) {
    return guard([&] {
        std::vector<std::array<u64, 3>> r(n);
        for (u64 i = 0; i < n; ++i) r[i] = {rels[3 * i], rels[3 * i + 1], rels[3 * i + 2]};   // (edge id, src, dst)
        auto e = t->t.remove_all(r);
        std::vector<u64> es, ed;
        for (auto& p : e) { es.push_back(p.first); ed.push_back(p.second); }
        *emptied_src = hand(es);
        *emptied_dst = hand(ed);
        *n_emptied = e.size();
        return 0;
    });
}
int fh_tn_op(fh_tn* t, int op, uint64_t a, uint64_t b) {
    return guard([&] {
        switch (op) {
            case 0: t->t.flush(); break;
            case 1: t->t.fold_oversized(); break;
            case 2: t->t.wait(); break;
            case 3: t->t.wait_fwd(); break;
            case 4: t->t.resize(a, b); break;
            default: throw GrbError(FGPU_INVALID, "fh_tn_op: unknown op");
        }
        return 0;
    });
}
int fh_tn_get(fh_tn* t, uint64_t src, uint64_t dst, uint64_t** ids, uint64_t* n) {
    return guard([&] {
        auto v = t->t.get(src, dst);
        *ids = hand(v);
        *n = v.size();
        return 0;
    });
}
int fh_tn_probe(fh_tn* t, int which, uint64_t src, uint64_t dst, uint64_t* val) {
    return guard([&] {
        std::optional<u64> v;
        if (which == 0) v = t->t.eff_get(src, dst);                     // eff_get_for_test
        else if (which == 1) { t->t.fwd_m().wait(); v = t->t.fwd_m().get(src, dst); }
        else if (which == 2) { Matrix e = t->t.extract(); e.wait(); v = e.get(src, dst); }
        else throw GrbError(FGPU_INVALID, "fh_tn_probe: which must be 0 (effective), 1 (m) or 2 (extract)");
        if (!v) return (int)FGPU_NO_VALUE;
        *val = *v;
        return 0;
    });
}
int fh_tn_state(fh_tn* t, uint64_t out[8]) {
    return guard([&] {
        out[7] = t->t.fwd_m().pending() ? 1 : 0;     // read BEFORE anything waits (resize_leaves_base_materialized)
        t->t.wait_fwd();
        out[0] = t->t.fwd_m().nvals();
        out[1] = t->t.fwd_dp().nvals();
        out[2] = t->t.fwd_dm().nvals();
        out[3] = t->t.multi_pairs();
        out[4] = t->t.matrix_t().extract().nvals();
        out[5] = t->t.me_nvals();
        out[6] = t->t.edge_count();
        return 0;
    });
}

int fh_tn_encode(fh_tn* t, uint8_t** bytes, uint64_t* len) {
    return guard([&] {
        ByteWriter w;
        t->t.encode(w);
        uint8_t* out = (uint8_t*)malloc(w.buf.size() ? w.buf.size() : 1);
        if (!out) throw GrbError(FGPU_OOM, "out of host memory");
        memcpy(out, w.buf.data(), w.buf.size());
        *bytes = out;
        *len = w.buf.size();
        return 0;
    });
}
int fh_tn_decode(fh_ctx* ctx, const uint8_t* bytes, uint64_t len, fh_tn** out, uint64_t* consumed) {
    return guard([&] {
        ByteReader r(bytes, len);
        Tensor t = Tensor::decode(ctx->c, r);
        t.rebuild_backward();                              // what the reference's caller does after decode (:1193-1195)
        *out = new fh_tn{std::move(t)};
        *consumed = r.pos;
        return 0;
    });
}

int fh_graph_layer_iter(fh_graph* g, int64_t type_id, int which, uint64_t** rows, uint64_t** cols, uint64_t** vals,
                        uint64_t* n) {
    return guard([&] {
        const Matrix* m;
        if (type_id < 0) {
            const VersionedMatrix& a = g->g.adjacency_matrix();
            a.wait();
            m = which == 0 ? &a.m() : which == 1 ? &a.dp() : &a.dm();
        } else {
            const Tensor& t = g->g.relationship_tensors().at((size_t)type_id);
            t.wait_fwd();
            m = which == 0 ? &t.fwd_m() : which == 1 ? &t.fwd_dp() : &t.fwd_dm();
        }
        auto es = m->iter(0, ~0ull);
        std::vector<u64> r, c, v;
        for (auto& e : es) { r.push_back(e.row); c.push_back(e.col); v.push_back(e.val); }
        *rows = hand(r);
        *cols = hand(c);
        *vals = hand(v);
        *n = es.size();
        return 0;
    });
}

// ---- operators -----------------------------------------------------------------------------------------------
static Value to_value(int64_t x) {
    if (x >= 0) return Value::node((u64)x);
    if (x == -2) return Value::null();
    return Value{};
}

// the (row, from, to, edge) columns of an operator's rows, handed out
static void hand_edge_rows(const CondTraverseOp::EdgeRows& rows, uint64_t** out_row, uint64_t** out_from, uint64_t** out_to,
                           uint64_t** out_edge, uint64_t* n) {
    *out_row = hand(rows.row);
    *out_from = hand(rows.from);
    *out_to = hand(rows.to);
    *out_edge = hand(rows.edge);
    *n = rows.size();
}

static CondVarLenTraverseOp var_len_op(const char* types, const char* dst_labels, int reversed, int bidirectional, uint32_t min_hops,
                                       uint32_t max_hops, int emit_path, int prune) {
    CondVarLenTraverseOp op;
    op.types = csv(types);
    op.dst_labels = csv(dst_labels);
    op.reversed = reversed != 0;
    op.bidirectional = bidirectional != 0;
    op.min_hops = min_hops;
    op.max_hops = max_hops;
    op.emit_path = emit_path != 0;
    op.prune = prune != 0;
    return op;
}

// VarLenRows flattened: the endpoints, the paths end to end and rows + 1 offsets into them.  The columns are reserved up
// front for the batch binding's sake, whose calls hand out very many rows.
static void hand_var_len_rows(const std::vector<VarLenRow>& rows, uint64_t** out_from, uint64_t** out_to, uint64_t** path,
                              uint64_t** path_off, uint64_t* n) {
    std::vector<u64> f, t, p, off{0};
    f.reserve(rows.size());
    t.reserve(rows.size());
    off.reserve(rows.size() + 1);
    for (auto& r : rows) {
        f.push_back(r.from);
        t.push_back(r.to);
        p.insert(p.end(), r.path.begin(), r.path.end());
        off.push_back(p.size());
    }
    *out_from = hand(f);
    *out_to = hand(t);
    *path = hand(p);
    *path_off = hand(off);
    *n = rows.size();
}

uint64_t fh_last_op_ns(void) { return g_last_op_ns; }

int fh_cond_traverse_eligible(const char* spec) { return parse_spec(spec).batched_eligible() ? 1 : 0; }

int fh_cond_traverse_batch(fh_graph* g, const char* spec, const int64_t* src, const int64_t* to_bound, uint64_t k,
                           int* batched, uint64_t** out_row, uint64_t** out_dest, int64_t** out_edge, uint64_t* n,
                           uint64_t** null_rows, uint64_t* n_null, uint64_t* flops) {
    return guard([&] {
        CondTraverseOp op = parse_spec(spec);
        std::vector<Value> s(k), tb(k);
        for (u64 i = 0; i < k; ++i) {
            s[i] = to_value(src[i]);
            if (to_bound) tb[i] = to_value(to_bound[i]);
        }
        // result columns keep their capacity between calls, as an operator's own batch buffers would: a fresh
        // 40 MB vector per call is mostly page faults (29 ms against 8 for a 4.9 M-row batch)
        static thread_local ExpandedRows rows;
        static thread_local std::vector<u64> nulls;
        u64 fl = 0;
        bool ok = timed([&] { return op.expand_batch(g->g, s, to_bound ? &tb : nullptr, rows, nulls, &fl); });
        *batched = ok ? 1 : 0;
        const size_t n_rows = rows.size();
        int64_t* e = (int64_t*)malloc((rows.size() ? rows.size() : 1) * sizeof(int64_t));
        if (rows.edge.empty()) memset(e, 0xFF, (rows.size() ? rows.size() : 1) * sizeof(int64_t));   // -1: none
        else memcpy(e, rows.edge.data(), rows.size() * sizeof(int64_t));
        if (rows.pinned()) {                                 // the harness wants malloc'ed u64 arrays: copy out of the pinned columns
            const size_t nn = rows.size();
            u64* r_ = (u64*)malloc((nn ? nn : 1) * sizeof(u64));
            u64* d_ = (u64*)malloc((nn ? nn : 1) * sizeof(u64));
            for (size_t q = 0; q < nn; ++q) { r_[q] = rows.row_at(q); d_[q] = rows.dest_at(q); }
            *out_row = r_;
            *out_dest = d_;
            rows.release_pinned();                           // (not kept across calls: the context may be gone before this thread is)
        } else {
            *out_row = hand(rows.active_row);
            *out_dest = hand(rows.dest);
        }
        *out_edge = e;
        *n = n_rows;
        *null_rows = hand(nulls);
        *n_null = nulls.size();
        if (flops) *flops = fl;
        return 0;
    });
}

int fh_cond_traverse_rows(fh_graph* g, const char* spec, const int64_t* from_ids, const int64_t* to_ids,
                          const int64_t* dedup_src, uint64_t k, int transposed, const uint64_t* used_edges,
                          uint64_t n_used, uint64_t** out_row, uint64_t** out_from, uint64_t** out_to,
                          uint64_t** out_edge, uint64_t* n) {
    return guard([&] {
        CondTraverseOp op = parse_spec(spec);
        CondTraverseOp::BidirDedup dd;                       // one input batch: fresh dedup state (:1268-1270)
        std::vector<u64> used(used_edges, used_edges + (used_edges ? n_used : 0));
        CondTraverseOp::EdgeRows rows;
        for (u64 i = 0; i < k; ++i) {
            if (from_ids[i] == -2 || to_ids[i] == -2) continue;   // bound to a non-node: no rows (:792-803)
            std::vector<std::array<u64, 3>> out;
            const bool dedup = dedup_src != nullptr;
            op.expand_row(g->g, from_ids[i] >= 0 ? std::optional<u64>((u64)from_ids[i]) : std::nullopt,
                          to_ids[i] >= 0 ? std::optional<u64>((u64)to_ids[i]) : std::nullopt, transposed != 0, used, out,
                          dedup ? &dd : nullptr,
                          dedup && dedup_src[i] >= 0 ? std::optional<u64>((u64)dedup_src[i]) : std::nullopt);
            for (auto& x : out) rows.push(i, x[0], x[1], x[2]);
        }
        hand_edge_rows(rows, out_row, out_from, out_to, out_edge, n);
        return 0;
    });
}

int fh_cond_traverse_edges_batch(fh_graph* g, const char* spec, const int64_t* from_ids, const int64_t* to_ids, uint64_t k,
                                 int transposed, int cross_row_dedup, const uint64_t* used_edges, uint64_t n_used, int* batched,
                                 uint64_t** out_row, uint64_t** out_from, uint64_t** out_to, uint64_t** out_edge, uint64_t* n,
                                 uint64_t** null_rows, uint64_t* n_null, uint64_t stats[8]) {
    return guard([&] {
        CondTraverseOp op = parse_spec(spec);
        std::vector<Value> f(k), t(k);
        for (u64 i = 0; i < k; ++i) {
            f[i] = to_value(from_ids[i]);
            t[i] = to_value(to_ids[i]);
        }
        CondTraverseOp::EdgeRows rows;
        std::vector<u64> nulls;
        bool ok = timed([&] {
            return op.expand_batch_edges(g->g, f, t, transposed != 0, used_edges, used_edges ? n_used : 0, rows, nulls, stats,
                                         cross_row_dedup != 0);
        });
        *batched = ok ? 1 : 0;
        hand_edge_rows(rows, out_row, out_from, out_to, out_edge, n);
        *n_null = nulls.size();
        *null_rows = hand(nulls);
        return 0;
    });
}

static void hand_semi_stats(const SemiApplyOp::Stats& st, int* tier, uint64_t stats[5]) {
    if (tier) *tier = st.tier;
    if (stats) {
        for (int j = 0; j < 4; ++j) stats[j] = st.device[j];
        stats[4] = st.calls;
    }
}

int fh_semi_apply(fh_graph* g, const char* spec, int anti, int device_exists, const int64_t* from_ids, const int64_t* to_ids,
                  uint64_t k, int transposed, uint64_t** passing, uint64_t* n, int* tier, uint64_t stats[5]) {
    return guard([&] {
        SemiApplyOp op;
        op.pattern = parse_spec(spec);
        op.anti = anti != 0;
        op.device_exists = device_exists != 0;
        std::vector<Value> f(k), t(k);
        for (u64 i = 0; i < k; ++i) {
            f[i] = to_value(from_ids[i]);
            if (to_ids) t[i] = to_value(to_ids[i]);
        }
        std::vector<u64> pass;
        SemiApplyOp::Stats st;
        timed([&] { op.filter_batch(g->g, f, to_ids ? &t : nullptr, transposed != 0, pass, &st); return 0; });
        *passing = hand(pass);
        *n = pass.size();
        hand_semi_stats(st, tier, stats);
        return 0;
    });
}

int fh_or_apply(fh_graph* g, const char* const* specs, const uint8_t* const* columns, const int* anti, const int* transposed,
                int n_branches, int device_exists, const int64_t* from_ids, const int64_t* to_ids, uint64_t k,
                uint64_t** passing, uint64_t* n, int* tiers, uint64_t* stats) {
    return guard([&] {
        OrApplyMultiplexerOp op;
        for (int b = 0; b < n_branches; ++b) {
            OrApplyMultiplexerOp::Branch br;
            br.anti = anti && anti[b];
            br.transposed = transposed && transposed[b];
            if (specs && specs[b]) {
                br.semi.emplace();
                br.semi->pattern = parse_spec(specs[b]);
                br.semi->device_exists = device_exists != 0;
            } else {
                if (!columns || !columns[b]) throw GrbError(FGPU_NULL_POINTER, "fh_or_apply: a branch needs a spec or a column");
                br.column.assign(columns[b], columns[b] + k);
            }
            op.branches.push_back(std::move(br));
        }
        std::vector<Value> f(k), t(k);
        for (u64 i = 0; i < k; ++i) {
            f[i] = to_value(from_ids[i]);
            if (to_ids) t[i] = to_value(to_ids[i]);
        }
        std::vector<u64> pass;
        std::vector<SemiApplyOp::Stats> st;
        timed([&] { op.filter_batch(g->g, f, to_ids ? &t : nullptr, pass, &st); return 0; });
        *passing = hand(pass);
        *n = pass.size();
        for (int b = 0; b < n_branches; ++b) hand_semi_stats(st[b], tiers ? tiers + b : nullptr, stats ? stats + 5 * b : nullptr);
        return 0;
    });
}

int fh_cond_traverse_row(fh_graph* g, const char* spec, int64_t from_id, int64_t to_id, int transposed,
                         uint64_t** out_from, uint64_t** out_to, uint64_t** out_edge, uint64_t* n) {
    uint64_t* rows = nullptr;
    int rc = fh_cond_traverse_rows(g, spec, &from_id, &to_id, nullptr, 1, transposed, nullptr, 0, &rows, out_from, out_to,
                                   out_edge, n);
    if (rc == 0) fh_free(rows);
    return rc;
}

int fh_expand_into(fh_graph* g, const char* types, int bidirectional, int emit_relationship, int batched,
                   const uint64_t* srcs, const uint64_t* dsts, uint64_t k, uint64_t** out_row, uint64_t** out_src,
                   uint64_t** out_dst, uint64_t** out_edge, uint64_t* n) {
    return guard([&] {
        ExpandIntoOp op;
        op.types = csv(types);
        op.bidirectional = bidirectional != 0;
        op.emit_relationship = emit_relationship != 0;
        std::vector<std::vector<std::array<u64, 3>>> per_row(k);
        if (batched) {
            op.expand_batch(g->g, std::vector<u64>(srcs, srcs + k), std::vector<u64>(dsts, dsts + k), per_row);
        } else {
            for (u64 i = 0; i < k; ++i) per_row[i] = op.expand_row(g->g, srcs[i], dsts[i]);
        }
        CondTraverseOp::EdgeRows rows;                       // (src, dst) in the from / to columns
        for (u64 i = 0; i < k; ++i)
            for (auto& x : per_row[i]) rows.push(i, x[0], x[1], x[2]);
        hand_edge_rows(rows, out_row, out_src, out_dst, out_edge, n);
        return 0;
    });
}

int fh_var_len_traverse(fh_graph* g, const char* types, const char* dst_labels, int reversed, int bidirectional,
                        uint32_t min_hops, uint32_t max_hops, uint64_t start, int64_t dest, int emit_path, int prune,
                        uint64_t** out_from, uint64_t** out_to, uint64_t** path, uint64_t** path_off, uint64_t* n,
                        uint64_t stats[3]) {
    return guard([&] {
        const CondVarLenTraverseOp op = var_len_op(types, dst_labels, reversed, bidirectional, min_hops, max_hops, emit_path, prune);
        std::vector<VarLenRow> rows;
        VarLenStats st;
        op.expand_row(g->g, start, dest >= 0 ? std::optional<u64>((u64)dest) : std::nullopt, rows, &st);
        hand_var_len_rows(rows, out_from, out_to, path, path_off, n);
        if (stats) { stats[0] = st.frames; stats[1] = st.pruned; stats[2] = st.reach_products; }
        return 0;
    });
}

int fh_var_len_traverse_batch(fh_graph* g, const char* types, const char* dst_labels, int reversed, int bidirectional,
                              uint32_t min_hops, uint32_t max_hops, const uint64_t* starts, const int64_t* dests, uint64_t k,
                              int emit_path, int prune, uint64_t device_budget, uint64_t** out_row, uint64_t** out_from,
                              uint64_t** out_to, uint64_t** path, uint64_t** path_off, uint64_t* n, uint64_t stats[3],
                              uint64_t* device_calls) {
    return guard([&] {
        CondVarLenTraverseOp op = var_len_op(types, dst_labels, reversed, bidirectional, min_hops, max_hops, emit_path, prune);
        if (device_budget) op.device_budget = device_budget;
        std::vector<std::optional<u64>> d;
        if (dests)
            for (u64 i = 0; i < k; ++i) d.push_back(dests[i] >= 0 ? std::optional<u64>((u64)dests[i]) : std::nullopt);
        std::vector<u64> rows_of;
        std::vector<VarLenRow> rows;
        VarLenStats st;
        u64 calls = 0;
        timed([&] { op.expand_batch(g->g, std::vector<u64>(starts, starts + k), d, rows_of, rows, &st, &calls); return 0; });
        *out_row = hand(rows_of);
        hand_var_len_rows(rows, out_from, out_to, path, path_off, n);
        if (stats) { stats[0] = st.frames; stats[1] = st.pruned; stats[2] = st.reach_products; }
        if (device_calls) *device_calls = calls;
        return 0;
    });
}

// AllShortestPathsOp over one input row: the paths flattened as relationship ids plus n_paths + 1 offsets
int fh_all_shortest_paths(fh_graph* g, const char* types, int bidirectional, int reversed, uint32_t max_hops, uint64_t src,
                          uint64_t dst, uint64_t limit, int64_t* length, uint64_t** edges, uint64_t** path_off, uint64_t* n_paths) {
    return guard([&] {
        AllShortestPathsOp op;
        op.types = csv(types);
        op.bidirectional = bidirectional != 0;
        op.reversed = reversed != 0;
        op.max_hops = max_hops;
        int64_t len = -1;
        const std::vector<std::vector<u64>> paths = timed([&] { return op.expand_row(g->g, src, dst, limit, &len); });
        std::vector<u64> e, off{0};
        for (auto& p : paths) {
            e.insert(e.end(), p.begin(), p.end());
            off.push_back(e.size());
        }
        *length = len;
        *edges = hand(e);
        *path_off = hand(off);
        *n_paths = paths.size();
        return 0;
    });
}

// AllShortestPathsOp over a parent batch of rows: the paths of all rows flattened, path_off cuts them into paths, row_off the
// paths into rows
int fh_all_shortest_paths_batch(fh_graph* g, const char* types, int bidirectional, int reversed, uint32_t max_hops,
                                const uint64_t* srcs, const uint64_t* dsts, uint64_t count, uint64_t limit, int64_t* lengths,
                                uint64_t** edges, uint64_t** path_off, uint64_t* row_off, uint64_t* device_calls) {
    return guard([&] {
        AllShortestPathsOp op;
        op.types = csv(types);
        op.bidirectional = bidirectional != 0;
        op.reversed = reversed != 0;
        op.max_hops = max_hops;
        const std::vector<u64> s(srcs, srcs + count), d(dsts, dsts + count);
        std::vector<int64_t> len;
        u64 calls = 0;
        const auto rows = timed([&] { return op.expand_batch(g->g, s, d, limit, &len, &calls); });
        std::vector<u64> e, off{0};
        row_off[0] = 0;
        for (u64 i = 0; i < count; ++i) {
            for (auto& p : rows[i]) {
                e.insert(e.end(), p.begin(), p.end());
                off.push_back(e.size());
            }
            row_off[i + 1] = off.size() - 1;
            lengths[i] = len[i];
        }
        *edges = hand(e);
        *path_off = hand(off);
        if (device_calls) *device_calls = calls;
        return 0;
    });
}

// shortestPath(): an endpoint of the C surface is a node id, -1 for Null, anything below for a value that is not a node
static Value sp_value(int64_t v) { return v >= 0 ? Value::node((u64)v) : v == -1 ? Value::null() : Value{Value::Other, 0}; }
static ShortestPathFn sp_fn(const char* types, int directed, uint32_t min_hops, uint32_t max_hops) {
    ShortestPathFn fn;
    fn.types = csv(types);
    fn.directed = directed != 0;
    fn.min_hops = min_hops;
    fn.max_hops = max_hops;
    return fn;
}

int fh_shortest_path(fh_graph* g, const char* types, int directed, uint32_t min_hops, uint32_t max_hops, int64_t src, int64_t dst,
                     int* is_null, uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, uint64_t* n_edges) {
    return guard([&] {
        const ShortestPathFn fn = sp_fn(types, directed, min_hops, max_hops);
        const ShortestPathFn::Path p = timed([&] { return fn.eval_row(g->g, sp_value(src), sp_value(dst)); });
        *is_null = p.null ? 1 : 0;
        *nodes = hand(p.nodes);
        *n_nodes = p.nodes.size();
        *edges = hand(p.edges);
        *n_edges = p.edges.size();
        return 0;
    });
}

int fh_shortest_path_batch(fh_graph* g, const char* types, int directed, uint32_t min_hops, uint32_t max_hops, const int64_t* srcs,
                           const int64_t* dsts, uint64_t count, uint8_t* is_null, uint64_t** nodes, uint64_t* node_off,
                           uint64_t** edges, uint64_t* edge_off, uint64_t* device_calls) {
    return guard([&] {
        const ShortestPathFn fn = sp_fn(types, directed, min_hops, max_hops);
        std::vector<Value> s, d;
        for (u64 i = 0; i < count; ++i) { s.push_back(sp_value(srcs[i])); d.push_back(sp_value(dsts[i])); }
        u64 calls = 0;
        const std::vector<ShortestPathFn::Path> rows = timed([&] { return fn.eval_batch(g->g, s, d, &calls); });
        std::vector<u64> nv, ev;
        node_off[0] = edge_off[0] = 0;
        for (u64 i = 0; i < count; ++i) {
            is_null[i] = rows[i].null ? 1 : 0;
            nv.insert(nv.end(), rows[i].nodes.begin(), rows[i].nodes.end());
            ev.insert(ev.end(), rows[i].edges.begin(), rows[i].edges.end());
            node_off[i + 1] = nv.size();
            edge_off[i + 1] = ev.size();
        }
        *nodes = hand(nv);
        *edges = hand(ev);
        if (device_calls) *device_calls = calls;
        return 0;
    });
}

int fh_node_degrees(fh_graph* g, const char* types, int incoming, const uint64_t* ids, uint64_t k, int mode, uint64_t* out,
                    uint64_t* device_calls) {
    return guard([&] {
        if (mode != 0 && mode != 1) throw std::invalid_argument("fh_node_degrees: mode must be 0 (per row) or 1 (batch)");
        DegreeFn fn;
        fn.incoming = incoming != 0;
        fn.types = csv(types);
        const std::vector<u64> v(ids, ids + k);
        u64 calls = 0;
        const std::vector<u64> deg = timed([&] {
            if (mode == 1) return fn.eval_batch(g->g, v, &calls);
            for (u64 id : v)   // (every id before the first result, as the batch checks them)
                if (id >= g->g.node_cap())
                    throw std::out_of_range("fh_node_degrees: node id " + std::to_string(id) + " is at or past the node capacity");
            std::vector<u64> rows(k);
            for (u64 i = 0; i < k; ++i) rows[i] = fn.eval_row(g->g, v[i]);
            return rows;
        });
        if (k) memcpy(out, deg.data(), k * sizeof(u64));
        if (device_calls) *device_calls = calls;
        return 0;
    });
}

int fh_node_degrees_all(fh_graph* g, const char* types, int incoming, uint64_t** out, uint64_t* n) {
    return guard([&] {
        DegreeFn fn;
        fn.incoming = incoming != 0;
        fn.types = csv(types);
        const std::vector<u64> deg = timed([&] { return fn.eval_all(g->g); });
        *out = hand(deg);
        *n = deg.size();
        return 0;
    });
}

// fh_algo_bfs and fh_algo_bfs_multi: one call but for the gang (nullptr: the graph's own context); only the single-context
// entry is a timed operator
static int algo_bfs_c(fh_graph* g, const std::vector<Context*>* gang, int64_t source, int64_t max_depth, const char* rel_type,
                      int want_edges, int* has_row, uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, uint64_t* n_edges) {
    auto run = [&] {
        return algo_bfs(g->g, source >= 0 ? std::optional<u64>((u64)source) : std::nullopt, max_depth,
                        rel_type ? std::optional<std::string>(rel_type) : std::nullopt, want_edges != 0, gang);
    };
    BfsResult r = gang ? run() : timed(run);
    *has_row = r.has_row ? 1 : 0;
    *nodes = hand(r.nodes);
    *n_nodes = r.nodes.size();
    *edges = hand(r.edges);
    *n_edges = r.edges.size();
    return 0;
}

int fh_algo_bfs(fh_graph* g, int64_t source, int64_t max_depth, const char* rel_type, int want_edges, int* has_row,
                uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, uint64_t* n_edges) {
    return guard([&] {
        return algo_bfs_c(g, nullptr, source, max_depth, rel_type, want_edges, has_row, nodes, n_nodes, edges, n_edges);
    });
}

int fh_algo_bfs_multi(fh_graph* g, fh_ctx* const* gang, int n_gang, int64_t source, int64_t max_depth,
                      const char* rel_type, int want_edges, int* has_row, uint64_t** nodes, uint64_t* n_nodes,
                      uint64_t** edges, uint64_t* n_edges) {
    return guard([&] {
        std::vector<Context*> cs;
        for (int i = 0; i < n_gang; ++i) cs.push_back(&gang[i]->c);
        return algo_bfs_c(g, &cs, source, max_depth, rel_type, want_edges, has_row, nodes, n_nodes, edges, n_edges);
    });
}

// ---- v19 matrix payload (serialize.cpp) -------------------------------------------------------------------
// CPU-only parse of a container payload: dims, flags and the index / value arrays it carries
int fh_container_parse(const uint8_t* bytes, uint64_t len, uint64_t* dims /* nrows, ncols, nvals, hyper, valued, consumed */,
                       uint64_t** p, uint64_t* np, uint64_t** h, uint64_t* nh, uint64_t** i, uint64_t** x) {
    return guard([&] {
        ByteReader r(bytes, len);
        ContainerData c = parse_container(r);
        dims[0] = c.nrows; dims[1] = c.ncols; dims[2] = c.nvals; dims[3] = c.hyper ? 1 : 0; dims[4] = c.valued ? 1 : 0;
        dims[5] = r.pos;
        *p = hand(c.p); *np = c.p.size();
        *h = hand(c.h); *nh = c.h.size();
        *i = hand(c.i);
        *x = hand(c.x);
        return 0;
    });
}
int fh_mat_decode(fh_ctx* ctx, const uint8_t* bytes, uint64_t len, fh_mat** out, uint64_t* consumed) {
    return guard([&] {
        ByteReader r(bytes, len);
        *out = new fh_mat{Matrix::decode(ctx->c, r)};
        if (consumed) *consumed = r.pos;
        return 0;
    });
}
int fh_mat_encode(fh_mat* m, uint8_t** bytes, uint64_t* len) {
    return guard([&] {
        ByteWriter w;
        m->m.encode(w);
        uint8_t* out = (uint8_t*)malloc(w.buf.size() ? w.buf.size() : 1);
        memcpy(out, w.buf.data(), w.buf.size());
        *bytes = out;
        *len = w.buf.size();
        return 0;
    });
}

// build_adjacency_matrix / build_symmetric_adjacency_matrix (graph.rs:3870-3907); types = comma list, "" = all
int fh_graph_build_adjacency(fh_graph* g, const char* types, int symmetric, fh_mat** out) {
    return guard([&] {
        const std::vector<std::string> ts = csv(types);
        *out = new fh_mat{symmetric ? g->g.build_symmetric_adjacency_matrix(ts) : g->g.build_adjacency_matrix(ts)};
        return 0;
    });
}

// plan text in, plan text out after fuse_anonymous_traverse; *spec (nullable) receives the runtime spec string
// (the fh_cond_traverse_batch format) of the CondTraverse node `lower_id` of the RESULT, or "" if lower_id < 0
int fh_plan_fuse(const char* plan_text, int lower_id, char** out_text, char** spec) {
    return guard([&] {
        Plan plan = parse_plan(plan_text ? plan_text : "");
        fuse_anonymous_traverse(plan);
        const std::string txt = print_plan(plan);
        *out_text = strdup(txt.c_str());
        if (spec) {
            std::string sp;
            if (lower_id >= 0 && (size_t)lower_id < plan.ops.size() && plan.ops[lower_id].kind == PlanOp::CondTraverse) {
                CondTraverseOp op = lower_cond_traverse(plan.ops[lower_id]);
                sp = "src=";
                for (size_t i = 0; i < op.src_labels.size(); ++i) sp += (i ? "," : "") + op.src_labels[i];
                for (auto& h : op.hops) {
                    sp += ";hop=";
                    for (size_t i = 0; i < h.types.size(); ++i) sp += (i ? "," : "") + h.types[i];
                    sp += "|";
                    for (size_t i = 0; i < h.dst_labels.size(); ++i) sp += (i ? "," : "") + h.dst_labels[i];
                }
                sp += std::string(";optional=") + (op.optional ? "1" : "0") + ";bind=" + (op.bind_relationship ? "1" : "0") +
                      ";emit=" + (op.emit_relationship ? "1" : "0") + ";bidir=" + (op.bidirectional ? "1" : "0") +
                      ";siblings=" + (op.has_sibling_edges ? "1" : "0") + ";attrs=" + (op.has_inline_attrs ? "1" : "0");
            }
            *spec = strdup(sp.c_str());
        }
        return 0;
    });
}

int fh_algo_pagerank(fh_graph* g, const char* label, const char* rel_type, uint64_t** nodes, double** scores,
                     uint64_t* n) {
    return guard([&] {
        PageRankResult r = timed([&] {
            return algo_pagerank(g->g, label ? std::optional<std::string>(label) : std::nullopt,
                                 rel_type ? std::optional<std::string>(rel_type) : std::nullopt);
        });
        *nodes = hand(r.nodes);
        *scores = hand(r.scores);
        *n = r.nodes.size();
        return 0;
    });
}

// algo.WCC: labels / types = comma lists, "" = all
int fh_algo_wcc(fh_graph* g, const char* labels, const char* types, uint64_t** nodes, int64_t** component_ids, uint64_t* n) {
    return guard([&] {
        WccResult r = timed([&] { return algo_wcc(g->g, csv(labels), csv(types)); });
        *nodes = hand(r.nodes);
        *component_ids = hand(r.component_ids);
        *n = r.nodes.size();
        return 0;
    });
}

// algo.labelPropagation: labels / types = comma lists, "" = all
int fh_algo_cdlp(fh_graph* g, const char* labels, const char* types, int64_t max_iterations, uint64_t** nodes,
                 int64_t** community_ids, uint64_t* n) {
    return guard([&] {
        CdlpResult r = timed([&] { return algo_cdlp(g->g, csv(labels), csv(types), max_iterations); });
        *nodes = hand(r.nodes);
        *community_ids = hand(r.community_ids);
        *n = r.nodes.size();
        return 0;
    });
}

// algo.HarmonicCentrality: labels / types = comma lists, "" = all
int fh_algo_harmonic_centrality(fh_graph* g, const char* labels, const char* types, uint64_t** nodes, double** scores,
                                int64_t** reachable, uint64_t* n) {
    return guard([&] {
        HarmonicResult r = timed([&] { return algo_harmonic_centrality(g->g, csv(labels), csv(types)); });
        *nodes = hand(r.nodes);
        *scores = hand(r.scores);
        *reachable = hand(r.reachable);
        *n = r.nodes.size();
        return 0;
    });
}

// algo.MSF: labels / types = comma lists, "" = all; the trees as two CSR-like lists
int fh_algo_msf(fh_graph* g, const char* labels, const char* types, int maximize, const uint64_t* edge_ids, const double* weights,
                uint64_t n_weights, uint64_t* n_trees, uint64_t** node_off, uint64_t** nodes, uint64_t** edge_off,
                uint64_t** edges) {
    return guard([&] {
        MsfResult r = timed([&] { return algo_msf(g->g, csv(labels), csv(types), maximize != 0, edge_ids, weights, n_weights); });
        std::vector<u64> no(1, 0), nv, eo(1, 0), ev;
        for (size_t t = 0; t < r.tree_nodes.size(); ++t) {
            nv.insert(nv.end(), r.tree_nodes[t].begin(), r.tree_nodes[t].end());
            ev.insert(ev.end(), r.tree_edges[t].begin(), r.tree_edges[t].end());
            no.push_back(nv.size());
            eo.push_back(ev.size());
        }
        *n_trees = r.tree_nodes.size();
        *node_off = hand(no);
        *nodes = hand(nv);
        *edge_off = hand(eo);
        *edges = hand(ev);
        return 0;
    });
}

// the eight stats of the last fgpu_pair_weights call an algorithm made on g (fgpu.h), all 0 before the first
int fh_graph_pair_stats(fh_graph* g, uint64_t stats[8]) {
    return guard([&] {
        const std::array<u64, 8> st = g->g.pair_stats();
        std::copy(st.begin(), st.end(), stats);
        return 0;
    });
}

// algo.maxFlow: labels / types = comma lists; the capacity attribute as (edge_ids[k], caps[k])
int fh_algo_maxflow(fh_graph* g, const char* labels, const char* types, const uint64_t* sources, uint64_t n_sources,
                    const uint64_t* targets, uint64_t n_targets, int has_attribute, const uint64_t* edge_ids, const double* caps,
                    uint64_t n_caps, int has_default, double default_capacity, uint64_t** nodes, uint64_t* n_nodes,
                    uint64_t** edges, double** flows, uint64_t* n_edges, double* max_flow) {
    return guard([&] {
        const std::vector<u64> src(sources, sources + (sources ? n_sources : 0)), dst(targets, targets + (targets ? n_targets : 0));
        MaxFlowResult r = timed([&] {
            return algo_maxflow(g->g, csv(labels), csv(types), src, dst, has_attribute != 0, edge_ids, caps, n_caps, has_default != 0,
                                default_capacity);
        });
        *nodes = hand(r.nodes);
        *n_nodes = r.nodes.size();
        *edges = hand(r.edges);
        *flows = hand(r.flows);
        *n_edges = r.edges.size();
        *max_flow = r.max_flow;
        return 0;
    });
}

// algo.SPpaths, the single cheapest path: types = a comma list, "" = all; direction 0 outgoing, 1 incoming, 2 both
int fh_algo_sp_paths(fh_graph* g, uint64_t source, uint64_t target, const char* types, int direction, const uint64_t* w_edge_ids,
                     const double* w_vals, uint64_t n_w, const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, int* found,
                     uint64_t** nodes, uint64_t* n_nodes, uint64_t** edges, double* weight, double* cost) {
    return guard([&] {
        if (direction < 0 || direction > 2) throw std::invalid_argument("fh_algo_sp_paths: direction must be 0, 1 or 2");
        SpPathResult r = timed([&] {
            return algo_sp_paths(g->g, source, target, csv(types), (Direction)direction, w_edge_ids, w_vals, n_w, c_edge_ids, c_vals,
                                 n_c);
        });
        *found = r.found ? 1 : 0;
        *nodes = hand(r.nodes);
        *n_nodes = r.nodes.size();
        *edges = hand(r.edges);
        *weight = r.weight;
        *cost = r.cost;
        return 0;
    });
}

// algo.SPpaths in every shape and algo.SSpaths: the rows flattened — row r has edges[offsets[r] .. offsets[r + 1]) and the
// nodes[offsets[r] + r .. offsets[r + 1] + r + 1) (one node more than edges)
static PathQuery path_query(const char* who, const char* types, int direction, int64_t max_len, int has_max_cost, double max_cost,
                            int64_t path_count, const uint64_t* w_edge_ids, const double* w_vals, uint64_t n_w,
                            const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, int prune, uint64_t max_examined) {
    if (direction < 0 || direction > 2) throw std::invalid_argument(std::string(who) + ": direction must be 0, 1 or 2");
    PathQuery q;
    q.types = csv(types);
    q.dir = (Direction)direction;
    q.max_len = max_len < 0 || max_len >= (int64_t)UINT32_MAX ? UINT32_MAX : (uint32_t)max_len;
    if (has_max_cost) q.max_cost = max_cost;
    q.path_count = path_count;
    q.w_edge_ids = w_edge_ids; q.w_vals = w_vals; q.n_w = n_w;
    q.c_edge_ids = c_edge_ids; q.c_vals = c_vals; q.n_c = n_c;
    q.prune = prune != 0;
    q.max_examined = max_examined;
    return q;
}

static void hand_paths(const std::vector<PathRow>& rows, const PathEnumStats& st, uint64_t* n_rows, uint64_t** offsets,
                       uint64_t** nodes, uint64_t** edges, double** weights, double** costs, int64_t stats[4]) {
    std::vector<u64> off(1, 0), nv, ev;
    std::vector<double> w, c;
    for (const PathRow& r : rows) {
        nv.insert(nv.end(), r.nodes.begin(), r.nodes.end());
        ev.insert(ev.end(), r.edges.begin(), r.edges.end());
        off.push_back(ev.size());
        w.push_back(r.weight);
        c.push_back(r.cost);
    }
    *n_rows = rows.size();
    *offsets = hand(off);
    *nodes = hand(nv);
    *edges = hand(ev);
    *weights = hand(w);
    *costs = hand(c);
    if (stats) {
        stats[0] = (int64_t)st.examined;
        stats[1] = (int64_t)st.pruned_hops;
        stats[2] = (int64_t)st.pruned_weight;
        stats[3] = st.table_rows;
    }
}

int fh_algo_sp_paths_rows(fh_graph* g, uint64_t source, uint64_t target, const char* types, int direction, int64_t max_len,
                          int has_max_cost, double max_cost, int64_t path_count, const uint64_t* w_edge_ids, const double* w_vals,
                          uint64_t n_w, const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, int prune,
                          uint64_t max_examined, uint64_t* n_rows, uint64_t** offsets, uint64_t** nodes, uint64_t** edges,
                          double** weights, double** costs, int64_t stats[4]) {
    return guard([&] {
        const PathQuery q = path_query("fh_algo_sp_paths_rows", types, direction, max_len, has_max_cost, max_cost, path_count,
                                       w_edge_ids, w_vals, n_w, c_edge_ids, c_vals, n_c, prune, max_examined);
        PathEnumStats st;
        const std::vector<PathRow> rows = timed([&] { return algo_sp_paths_rows(g->g, source, target, q, &st); });
        hand_paths(rows, st, n_rows, offsets, nodes, edges, weights, costs, stats);
        return 0;
    });
}

int fh_algo_ss_paths(fh_graph* g, uint64_t source, const char* types, int direction, int64_t max_len, int has_max_cost,
                     double max_cost, int64_t path_count, const uint64_t* w_edge_ids, const double* w_vals, uint64_t n_w,
                     const uint64_t* c_edge_ids, const double* c_vals, uint64_t n_c, uint64_t max_examined, uint64_t* n_rows,
                     uint64_t** offsets, uint64_t** nodes, uint64_t** edges, double** weights, double** costs, int64_t stats[4]) {
    return guard([&] {
        const PathQuery q = path_query("fh_algo_ss_paths", types, direction, max_len, has_max_cost, max_cost, path_count, w_edge_ids,
                                       w_vals, n_w, c_edge_ids, c_vals, n_c, 0, max_examined);
        PathEnumStats st;
        const std::vector<PathRow> rows = timed([&] { return algo_ss_paths(g->g, source, q, &st); });
        hand_paths(rows, st, n_rows, offsets, nodes, edges, weights, costs, stats);
        return 0;
    });
}

// algo.betweenness: labels / types = comma lists, "" = all
int fh_algo_betweenness(fh_graph* g, const char* labels, const char* types, int64_t sampling_size, int64_t sampling_seed,
                        uint64_t** nodes, double** scores, uint64_t* n) {
    return guard([&] {
        BetweennessResult r = timed([&] { return algo_betweenness(g->g, csv(labels), csv(types), sampling_size, sampling_seed); });
        *nodes = hand(r.nodes);
        *scores = hand(r.scores);
        *n = r.nodes.size();
        return 0;
    });
}

int fh_betweenness_sources(uint64_t n_nodes, int64_t sampling_size, int64_t sampling_seed, uint64_t** out, uint64_t* n) {
    return guard([&] {
        const std::vector<u64> s = betweenness_sources(n_nodes, sampling_size, sampling_seed);
        *out = hand(s);
        *n = s.size();
        return 0;
    });
}

// vector indexes, db.idx.vector.queryNodes / queryRelationships, vec.*Distance
int fh_graph_vector_index_create(fh_graph* g, int is_edge, uint64_t label_or_type_id, const char* attr, uint64_t dim,
                                 const char* similarity) {
    return guard([&] { g->g.vector_index_create(is_edge != 0, label_or_type_id, attr ? attr : "", dim, similarity); return 0; });
}
int fh_graph_vector_index_drop(fh_graph* g, int is_edge, uint64_t label_or_type_id, const char* attr) {
    return guard([&] { return g->g.vector_index_drop(is_edge != 0, label_or_type_id, attr ? attr : "") ? 0 : 1; });
}
int fh_graph_vector_set_node(fh_graph* g, uint64_t label_id, const char* attr, uint64_t node, const float* vec, uint64_t n) {
    return guard([&] { g->g.vector_set_node(label_id, attr ? attr : "", node, vec, n); return 0; });
}
int fh_graph_vector_set_edge(fh_graph* g, uint64_t type_id, const char* attr, uint64_t src, uint64_t dst, uint64_t edge_id,
                             const float* vec, uint64_t n) {
    return guard([&] { g->g.vector_set_edge(type_id, attr ? attr : "", src, dst, edge_id, vec, n); return 0; });
}
int fh_graph_vector_unset_node(fh_graph* g, uint64_t label_id, const char* attr, uint64_t node) {
    return guard([&] { return g->g.vector_unset_node(label_id, attr ? attr : "", node) ? 0 : 1; });
}
int fh_graph_vector_unset_edge(fh_graph* g, uint64_t type_id, const char* attr, uint64_t edge_id) {
    return guard([&] { return g->g.vector_unset_edge(type_id, attr ? attr : "", edge_id) ? 0 : 1; });
}
int fh_vector_query_nodes(fh_graph* g, const char* label, const char* attr, int64_t k, const float* q, uint64_t qn,
                          uint64_t** ids, double** dist, uint64_t* n) {
    return guard([&] {
        VectorHits r = timed([&] { return g->g.vector_query(false, label ? label : "", attr ? attr : "", k, q, qn, 1); });
        *ids = hand(r.ids);
        *dist = hand(r.dist);
        *n = r.ids.size();
        return 0;
    });
}
int fh_vector_query_edges(fh_graph* g, const char* type, const char* attr, int64_t k, const float* q, uint64_t qn,
                          uint64_t** ids, double** dist, uint64_t** srcs, uint64_t** dsts, uint64_t* n) {
    return guard([&] {
        VectorHits r = timed([&] { return g->g.vector_query(true, type ? type : "", attr ? attr : "", k, q, qn, 1); });
        *ids = hand(r.ids);
        *dist = hand(r.dist);
        *srcs = hand(r.srcs);
        *dsts = hand(r.dsts);
        *n = r.ids.size();
        return 0;
    });
}
int fh_vector_query_nodes_batch(fh_graph* g, const char* label, const char* attr, int64_t k, const float* queries, uint64_t qn,
                                uint64_t nq, uint64_t** offsets, uint64_t** ids, double** dist) {
    return guard([&] {
        VectorHits r = timed([&] { return g->g.vector_query(false, label ? label : "", attr ? attr : "", k, queries, qn, nq); });
        *offsets = hand(r.offsets);
        *ids = hand(r.ids);
        *dist = hand(r.dist);
        return 0;
    });
}
int fh_vec_distance(const char* metric, const float* a, uint64_t na, const float* b, uint64_t nb, double* out) {
    return guard([&] { *out = vec_distance(vector_metric(metric), a, na, b, nb); return 0; });
}

}  // extern "C"
