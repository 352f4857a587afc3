// graph.cpp — the traversal-facing slice of graph.rs plus the operators that sit on it:
// CondTraverseOp::expand_batch / expand_row, ExpandIntoOp, algo.BFS.
#include <algorithm>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <unordered_set>
#include <cmath>

#include "host.hpp"

namespace falkor {

// ---- Graph ------------------------------------------------------------------------------------------
Graph::Graph(Context& ctx, u64 node_cap, u64 label_cap)
    : ctx_(&ctx), n_(node_cap), adj_(ctx, node_cap, node_cap), labels_(ctx, node_cap, label_cap) {}

LabelId Graph::add_label(const std::string& name) {
    auto it = label_ids_.find(name);
    if (it != label_ids_.end()) return it->second;
    LabelId id = label_ids_.size();
    if (id >= labels_.ncols()) labels_.resize(labels_.nrows(), labels_.ncols() * 2);
    label_ids_[name] = id;
    return id;
}

u64 Graph::add_type(const std::string& name) {
    auto it = type_ids_.find(name);
    if (it != type_ids_.end()) return it->second;
    u64 id = tensors_.size();
    tensors_.emplace_back(*ctx_, n_, n_);
    type_ids_[name] = id;
    return id;
}

std::optional<LabelId> Graph::label_id(const std::string& name) const {
    auto it = label_ids_.find(name);
    if (it == label_ids_.end()) return std::nullopt;
    return it->second;
}
std::optional<u64> Graph::type_id(const std::string& name) const {
    auto it = type_ids_.find(name);
    if (it == type_ids_.end()) return std::nullopt;
    return it->second;
}

void Graph::create_edge(u64 type, u64 src, u64 dst, u64 edge_id) {
    tensors_.at(type).set_all_from_slices({src}, {dst}, {edge_id});
    adj_.set_all({{src, dst}}, false);   // two edges may share one pair: NEW = false
}

void Graph::delete_edge(u64 type, u64 src, u64 dst, u64 edge_id) {
    auto emptied = tensors_.at(type).remove_all({{edge_id, src, dst}});
    if (!vec_indexes_.empty()) drop_entity_vectors(true, type, edge_id);   // (after the removal: an unknown type has thrown)
    if (emptied.empty()) return;
    for (auto& t : tensors_)
        if (t.eff_get(src, dst)) return;   // another type still connects the pair
    adj_.remove(src, dst);
}

void Graph::create_edges(u64 type, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                         const std::vector<u64>& ids) {
    tensors_.at(type).set_all_from_slices(srcs, dsts, ids);
    std::vector<std::pair<u64, u64>> pairs(srcs.size());
    for (size_t k = 0; k < srcs.size(); ++k) pairs[k] = {srcs[k], dsts[k]};
    adj_.set_all(pairs, false);
}

BulkStats Graph::bulk_insert_edges(u64 type, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                                   const std::vector<u64>& ids) {
    if (srcs.size() != dsts.size() || srcs.size() != ids.size())
        throw GrbError(FGPU_INVALID, "bulk_insert_edges: slices differ in length");
    return bulk_insert_edges(type, srcs.data(), dsts.data(), ids.data(), srcs.size());
}

BulkStats Graph::bulk_insert_edges(u64 type, const u64* srcs, const u64* dsts, const u64* ids, u64 n) {
    std::optional<Matrix> built;
    BulkStats bs = tensors_.at(type).bulk_insert(srcs, dsts, ids, n, &built);
    const u64 t0 = bulk_clock_ns();
    if (built) {
        adj_.union_base(*built);
    } else if (bs.fallback_edges) {
        std::vector<std::pair<u64, u64>> pairs(n);
        for (size_t k = 0; k < n; ++k) pairs[k] = {srcs[k], dsts[k]};
        adj_.set_all(pairs, false);
    }
    bs.phase_ns[3] = bulk_clock_ns() - t0;
    return bs;
}

AppendStats Graph::append_edges_bulk(u64 type, const u64* srcs, const u64* dsts, const u64* ids, u64 n) {
    std::optional<Matrix> built;
    AppendStats as = tensors_.at(type).append_bulk(srcs, dsts, ids, n, &built);
    const u64 t0 = bulk_clock_ns();
    if (built) adj_.union_base(*built);
    as.phase_ns[3] = bulk_clock_ns() - t0;
    return as;
}

std::vector<std::array<u64, 3>> Graph::delete_nodes_bulk(const std::vector<u64>& nodes, const std::vector<u64>& skip_ids,
                                                         DetachStats* stats) {
    std::vector<std::array<u64, 3>> out;
    DetachStats ds;
    if (nodes.empty()) {
        if (stats) *stats = ds;
        return out;
    }
    for (u64 v : nodes)
        if (v >= n_)
            throw GrbError(FGPU_INVALID, "delete_nodes_bulk: node " + std::to_string(v) + " is at or past the capacity " +
                                             std::to_string(n_));
    const std::unordered_set<u64> skip(skip_ids.begin(), skip_ids.end());
    ds.per_type.assign(tensors_.size(), 0);
    DetachCounts dc;
    for (size_t t = 0; t < tensors_.size(); ++t) {
        const u64 before = dc.removed;
        const size_t listed0 = out.size(), skipped0 = dc.skipped.size();
        auto rels = tensors_[t].detach_nodes(nodes, skip, &dc);
        out.insert(out.end(), rels.begin(), rels.end());
        ds.per_type[t] = dc.removed - before;
        if (!vec_indexes_.empty()) {   // every removed edge leaves the indexes of its type, as delete_edge makes it
            for (size_t k = listed0; k < out.size(); ++k) drop_entity_vectors(true, t, out[k][0]);
            for (size_t k = skipped0; k < dc.skipped.size(); ++k) drop_entity_vectors(true, t, dc.skipped[k]);
        }
    }
    ds.edges_removed = dc.removed;
    ds.edges_listed = out.size();
    ds.multi_pairs = dc.multi_pairs;
    ds.phase_ns[0] = dc.phase_ns[0];
    ds.phase_ns[1] = dc.phase_ns[1];
    u64 t0 = bulk_clock_ns();
    ds.label_entries = labels_.detach_base(nodes, 1);     // graph.rs:1753-1768
    ds.phase_ns[2] = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    ds.adjacency_entries = adj_.detach_base(nodes, 3);
    ds.phase_ns[3] = bulk_clock_ns() - t0;
    std::unordered_set<u64> seen;
    for (u64 v : nodes)
        if (seen.insert(v).second) delete_node(v);
    ds.nodes = seen.size();
    if (stats) *stats = ds;
    return out;
}

std::vector<std::array<u64, 3>> Graph::delete_edges_bulk(const u64* types, const u64* srcs, const u64* dsts, const u64* ids, u64 n,
                                                         EdgeDeleteStats* stats) {
    std::vector<std::array<u64, 3>> out;
    EdgeDeleteStats es;
    es.per_type.assign(tensors_.size(), 0);
    es.edges_named = n;
    // nothing moves before the whole batch is known to be addressable
    bool one_type = true;
    for (u64 k = 0; k < n; ++k) {
        if (types[k] >= tensors_.size())
            throw GrbError(FGPU_INVALID, "delete_edges_bulk: edge " + std::to_string(k) + " names the unknown relationship type " +
                                             std::to_string(types[k]));
        if (srcs[k] >= n_ || dsts[k] >= n_)
            throw GrbError(FGPU_INVALID, "delete_edges_bulk: edge " + std::to_string(k) + " = (" + std::to_string(srcs[k]) + ", " +
                                             std::to_string(dsts[k]) + ") is at or past the capacity " + std::to_string(n_));
        one_type = one_type && types[k] == types[0];
    }
    // group by type (graph.rs:2285-2301); a batch of one type is handed on as it came
    std::map<u64, std::vector<u64>> by_type;   // type id -> positions in the batch, in input order
    if (n && one_type) by_type[types[0]];
    else
        for (u64 k = 0; k < n; ++k) by_type[types[k]].push_back(k);
    std::vector<std::pair<u64, u64>> cand;   // pairs some tensor emptied
    RemoveCounts rc;
    std::vector<u64> gs, gd, gi;
    for (auto& grp : by_type) {
        const u64 t = grp.first;
        const std::vector<u64>& pos = grp.second;
        const u64 cnt = one_type ? n : pos.size();
        const u64 *s = srcs, *d = dsts, *i = ids;
        if (!one_type) {
            gs.resize(cnt); gd.resize(cnt); gi.resize(cnt);
            for (size_t k = 0; k < cnt; ++k) { gs[k] = srcs[pos[k]]; gd[k] = dsts[pos[k]]; gi[k] = ids[pos[k]]; }
            s = gs.data(); d = gd.data(); i = gi.data();
        }
        auto emptied = tensors_[t].remove_bulk(s, d, i, cnt, &rc);
        cand.insert(cand.end(), emptied.begin(), emptied.end());
        es.pairs_emptied += emptied.size();
        es.pairs_demoted += rc.demoted;
        const size_t listed0 = out.size();
        if (rc.hits == rc.removed) {   // as many hitting triples as edges that left: none is repeated
            for (size_t k = 0; k < cnt; ++k)
                if (rc.hit[k]) out.push_back({i[k], s[k], d[k]});
        } else {
            std::unordered_set<u64> listed;
            for (size_t k = 0; k < cnt; ++k)
                if (rc.hit[k] && listed.insert(i[k]).second) out.push_back({i[k], s[k], d[k]});
        }
        es.per_type[t] = out.size() - listed0;
        if (!vec_indexes_.empty())   // every named id leaves the indexes of its type, as delete_edge makes it
            for (size_t k = 0; k < cnt; ++k) drop_entity_vectors(true, t, i[k]);
    }
    es.edges_removed = out.size();
    for (int k = 0; k < 3; ++k) es.phase_ns[k] = rc.phase_ns[k];
    const u64 t0 = bulk_clock_ns();
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    if (!cand.empty() && tensors_.size() > 1) {   // another type may still connect the pair: one batched probe per tensor
        std::vector<u64> cs(cand.size()), cd(cand.size());
        for (size_t k = 0; k < cand.size(); ++k) { cs[k] = cand[k].first; cd[k] = cand[k].second; }
        std::vector<uint8_t> held(cand.size(), 0), present;
        for (auto& t : tensors_) {
            t.contains_batch(cs, cd, present);
            for (size_t k = 0; k < cand.size(); ++k) held[k] |= present[k];
        }
        size_t left = 0;
        for (size_t k = 0; k < cand.size(); ++k)
            if (!held[k]) cand[left++] = cand[k];
        cand.resize(left);
    }
    if (!cand.empty()) {
        std::vector<u64> mr(cand.size()), mc(cand.size());
        for (size_t k = 0; k < cand.size(); ++k) { mr[k] = cand[k].first; mc[k] = cand[k].second; }
        Matrix mask(*ctx_, Type::Bool, n_, n_);
        mask.build(mr, mc);
        const u64 before = adj_.nvals();
        adj_.remove_mask(mask);
        es.adjacency_entries = before - adj_.nvals();
    }
    es.phase_ns[3] = bulk_clock_ns() - t0;
    if (stats) *stats = es;
    return out;
}

void Graph::new_version() {
    adj_ = adj_.dup();
    labels_ = labels_.dup();
    for (auto& t : tensors_) t = t.dup();
}

void Graph::fold_oversized_deltas() {
    adj_.fold_oversized();
    labels_.fold_oversized();
    for (auto& t : tensors_) t.fold_oversized();
}

bool Graph::node_has_label_id(u64 node, LabelId l) const { return labels_.get(node, l).has_value(); }

std::optional<std::vector<LabelId>> Graph::resolve_label_ids(const std::vector<std::string>& labels) const {
    std::vector<LabelId> out;
    for (auto& l : labels) {
        auto id = label_id(l);
        if (!id) return std::nullopt;
        out.push_back(*id);
    }
    return out;
}

std::vector<u64> Graph::label_bitmap(const std::vector<LabelId>& ids) const {
    const u64 words = (n_ + 63) / 64;
    std::vector<u64> bits(words, ~0ull);
    if (n_ % 64) bits[words - 1] = (1ull << (n_ % 64)) - 1;
    if (ids.empty()) return bits;
    // the label matrix is node x label: its transpose has one row per label = the node set of that label
    VersionedMatrix lt = labels_.transpose();
    for (LabelId l : ids) {
        std::vector<u64> has(words, 0);
        for (auto& e : lt.iter(l, l)) has[e.col >> 6] |= 1ull << (e.col & 63);
        for (u64 w = 0; w < words; ++w) bits[w] &= has[w];
    }
    return bits;
}

Matrix Graph::build_relationship_matrix_unrestricted(const std::vector<u64>& type_ids) const {
    // graph.rs:2520-2549: the first type's extract, then for every further type
    //   m<!dm_t> U= pattern(m_t) ; m U= pattern(dp_t)
    if (type_ids.empty()) return adj_.extract();
    Matrix m = tensors_.at(type_ids[0]).extract();
    for (size_t k = 1; k < type_ids.size(); ++k) {
        const Tensor& t = tensors_.at(type_ids[k]);
        t.wait_fwd();
        m.set_pattern(&t.fwd_dm(), t.fwd_m(), Descriptor::C);
        m.set_pattern(nullptr, t.fwd_dp(), Descriptor::None);
    }
    return m;
}

Matrix Graph::build_adjacency_matrix(const std::vector<std::string>& types) const {
    if (types.empty()) return adj_.extract();                       // graph.rs:3874-3876
    if (types.size() == 1) {
        auto id = type_id(types[0]);
        return id ? tensors_[*id].extract() : Matrix(*ctx_, Type::Bool, n_, n_);
    }
    Matrix result(*ctx_, Type::Bool, n_, n_);
    for (auto& t : types)
        if (auto id = type_id(t)) {
            Matrix e = tensors_[*id].extract();
            result.element_wise_add(nullptr, nullptr, &e, Descriptor::None);
        }
    return result;
}

Matrix Graph::build_symmetric_adjacency_matrix(const std::vector<std::string>& types) const {
    // graph.rs:3898-3907: result = A (+) A'  (the undirected view WCC / CDLP / MSF run on)
    Matrix a = build_adjacency_matrix(types);
    Matrix at = a.transpose();
    Matrix result(*ctx_, Type::Bool, n_, n_);
    result.element_wise_add(nullptr, &a, &at, Descriptor::None);
    return result;
}

std::vector<u64> Graph::get_src_dest_relationships(u64 src, u64 dst, const std::vector<u64>& type_ids) const {
    std::vector<u64> out;
    for (u64 t : type_ids) {
        auto ids = tensors_.at(t).get(src, dst);
        out.insert(out.end(), ids.begin(), ids.end());
    }
    return out;
}

// ---- CondTraverse -------------------------------------------------------------------------------------
bool CondTraverseOp::batched_eligible() const {
    // cond_traverse.rs:308-316
    return !emit_relationship && !bidirectional && !has_sibling_edges && (hops.size() > 1 || !has_inline_attrs);
}

namespace {
// ---- type names -> tensor ids: every operator and procedure below resolves its relationship types through these two --------
// The known names among `names`, in the order listed, a name listed twice kept twice: the `filter_map` of
// get_node_relationships_by_type (graph.rs:1803-1810), build_relationship_matrix_unrestricted (graph.rs:2524-2527) and
// edge_type_indices (cond_traverse.rs:418-426).
std::vector<u64> named_type_ids(const Graph& g, const std::vector<std::string>& names) {
    std::vector<u64> ids;
    for (auto& t : names)
        if (auto id = g.type_id(t)) ids.push_back(*id);
    return ids;
}

// The tensors a type list scans: none named = every tensor in id order, else named_type_ids.  Names of which none is known
// scan NOTHING — what that means is the caller's: CondTraverse's no_match (`!names.empty() && ids.empty()`: a single unknown
// type, cond_traverse.rs:481-490, or an alternation of unknown names) returns before anything runs, the other operators run
// over an empty scan.
std::vector<u64> scanned_type_ids(const Graph& g, const std::vector<std::string>& names) {
    if (!names.empty()) return named_type_ids(g, names);
    std::vector<u64> ids(g.relationship_tensors().size());
    for (u64 t = 0; t < ids.size(); ++t) ids[t] = t;
    return ids;
}

// ---- device layers -----------------------------------------------------------------------------------------------------
// The three layers of a delta matrix as the device wants them: an empty delta goes as null.  `on_device` turns a layer into
// its device handle.  The VersionedMatrix forms wait on that matrix alone; a tensor's forward layers are waited on by the
// caller (wait_fwd() on the hot forward hop, wait() where `mt` is read too): which layers a site materialises is its choice.
struct Layers { const fgpu_mat *m, *dp, *dm; };

template <class F>
Layers layers_of(const Matrix& m, const Matrix& dp, const Matrix& dm, F on_device) {
    return {on_device(m), dp.nvals() ? on_device(dp) : nullptr, dm.nvals() ? on_device(dm) : nullptr};
}
const fgpu_mat* snapshot_of(const Matrix& x) { return x.snapshot(); }
template <class F>
Layers layers_of(const VersionedMatrix& v, F on_device) {   // the adjacency, a tensor's `mt`
    v.wait();
    return layers_of(v.m(), v.dp(), v.dm(), on_device);
}
Layers layers_of(const VersionedMatrix& v) { return layers_of(v, snapshot_of); }
Layers fwd_layers(const Tensor& t) {                         // after the caller's wait_fwd() or wait()
    return layers_of(t.fwd_m(), t.fwd_dp(), t.fwd_dm(), snapshot_of);
}

struct HopLayers {
    // keeps temporaries (materialized unions, transposes) alive for the duration of the call
    std::vector<Matrix> owned;
    std::vector<const fgpu_mat*> m, dp, dm;
    const fgpu_mat* keep(Matrix x) { owned.push_back(std::move(x)); return owned.back().snapshot(); }
    void push(Layers l) { m.push_back(l.m); dp.push_back(l.dp); dm.push_back(l.dm); }
};

// Matrix choice per hop (cond_traverse.rs:478-505): no type -> adjacency; one type -> that tensor's forward
// layers; an alternation -> materialized union of its known types with clean deltas (also when only one of them
// is known: the reference branches on the number of NAMES).  `transposed`: the structures build_transposed_iter walks
// (cond_traverse.rs:221-235), as device layers: the transposes of the adjacency layers (cached on their snapshots: paid
// once per matrix version), the tensor's own `mt` (kept by every insert / delete, Tensor::matrix_t), the transpose of the
// materialized alternation.  type_ids gets the tensors each hop scans.  Returns false for no_match.
bool hop_layers(const Graph& g, const std::vector<Hop>& hops, HopLayers& hl, std::vector<std::vector<u64>>& type_ids,
                bool transposed = false) {
    hl.owned.reserve(3 * hops.size());
    auto kept_transpose = [&](const Matrix& x) { return hl.keep(x.transpose()); };
    for (auto& h : hops) {
        type_ids.push_back(scanned_type_ids(g, h.types));
        const std::vector<u64>& ids = type_ids.back();
        if (!h.types.empty() && ids.empty()) return false;
        if (h.types.empty()) {
            const VersionedMatrix& a = g.adjacency_matrix();
            hl.push(transposed ? layers_of(a, kept_transpose) : layers_of(a));
        } else if (h.types.size() == 1) {
            const Tensor& t = g.relationship_tensors()[ids[0]];
            if (!transposed) t.wait_fwd();               // (the forward hop never materialises a pending transpose)
            hl.push(transposed ? layers_of(t.matrix_t()) : fwd_layers(t));
        } else {
            Matrix u = g.build_relationship_matrix_unrestricted(ids);
            hl.push({hl.keep(transposed ? u.transpose() : std::move(u)), nullptr, nullptr});
        }
    }
    return true;
}

// ok[c] = nodes[c] carries every label of lids: node_has_label_id for the whole list, one batch of probes per layer of the
// label matrix and label
void nodes_have_labels(const Graph& g, const std::vector<LabelId>& lids, const std::vector<u64>& nodes, std::vector<uint8_t>& ok) {
    ok.assign(nodes.size(), 1);
    if (lids.empty() || nodes.empty()) return;
    const VersionedMatrix& lab = g.node_labels_matrix();
    lab.wait();
    for (LabelId l : lids) {
        std::vector<u64> cols(nodes.size(), l);
        std::vector<uint8_t> in_m, in_dm, in_dp;
        lab.m().probe(nodes, cols, in_m, nullptr);
        lab.dm().probe(nodes, cols, in_dm, nullptr);
        lab.dp().probe(nodes, cols, in_dp, nullptr);
        for (size_t c = 0; c < nodes.size(); ++c)
            if (!((in_m[c] && !in_dm[c]) || (!in_m[c] && in_dp[c]))) ok[c] = 0;
    }
}

// The layers of every scanned tensor as they lie on the device, forward and transposed, with the multi-edge table: the seven
// parallel arrays fgpu_expand_edges and fgpu_expand_trails take.  Tensor::wait() materialises both directions.
struct TensorLayerArrays {
    std::vector<const fgpu_mat*> m, dp, dm, tm, tdp, tdm;
    std::vector<const fgpu_multi*> multi;
    size_t size() const { return m.size(); }
};
TensorLayerArrays gather(const Graph& g, const std::vector<u64>& tids) {
    TensorLayerArrays a;
    for (u64 t : tids) {
        const Tensor& ten = g.relationship_tensors()[t];
        ten.wait();
        const Layers f = fwd_layers(ten), b = layers_of(ten.matrix_t());
        a.m.push_back(f.m); a.dp.push_back(f.dp); a.dm.push_back(f.dm);
        a.tm.push_back(b.m); a.tdp.push_back(b.dp); a.tdm.push_back(b.dm);
        a.multi.push_back(ten.multi_table());
    }
    return a;
}

// OPTIONAL (cond_traverse.rs:737-747): the input rows i < k without an emission, ascending, appended to null_rows;
// row_of(r) = the input row of emission r < n_emitted
template <class RowOf>
void append_rows_without_emission(u64 k, size_t n_emitted, RowOf row_of, std::vector<u64>& null_rows) {
    std::vector<uint8_t> matched(k, 0);
    for (size_t r = 0; r < n_emitted; ++r) matched[row_of(r)] = 1;
    for (u64 i = 0; i < k; ++i)
        if (!matched[i]) null_rows.push_back(i);
}
}  // namespace

bool CondTraverseOp::expand_batch(const Graph& g, const std::vector<Value>& src, const std::vector<Value>* to_bound,
                                  ExpandedRows& rows, std::vector<u64>& null_rows, u64* flops) const {
    rows.clear();
    null_rows.clear();
    if (flops) *flops = 0;
    const u64 k = src.size();
    auto null_pad = [&]() {                  // OPTIONAL: the rows without an emission (:737-747); on no_match, every row
        if (optional) append_rows_without_emission(k, rows.size(), [&](size_t r) { return rows.row_at(r); }, null_rows);
        return true;
    };
    // FH_TIMING=1: phase times of every call on stderr (tools/bench_paths.py host)
    static const bool timing = getenv("FH_TIMING") != nullptr;
    auto tp = timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();   // no clock reads on the hot path
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[expand_batch] %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tp).count());
        tp = now;
    };
    HopLayers hl;
    std::vector<std::vector<u64>> type_ids;
    // A `transposed` operator has the matrix DESTINATION bound (select_scan_node swaps from / to): the reference declines
    // the batch there (:556-568) and walks row d of the transposed structure per row (:221-235, 840-870).  The device holds
    // those structures as matrices, so the same batch machinery runs over them — F[i, bound_i] = 1, one product with the
    // transposed layers, `src_labels` on the bound node, the hop's labels on the node it reaches, the representative edge
    // looked up as (reached, bound) — and gives what the per-row path gives row by row.  One hop only (a transposed operator
    // is never fused, fuse_anonymous_traverse.rs:118-122).
    if (transposed && hops.size() != 1) return false;
    if (!hop_layers(g, hops, hl, type_ids, transposed)) return null_pad();          // no_match: unknown type (:485-490)
    lap("hop_layers");
    auto last_dst = g.resolve_label_ids(hops.back().dst_labels);
    auto src_lids = g.resolve_label_ids(src_labels);
    if (!last_dst || !src_lids) return null_pad();                      // no_match: unknown label

    // F[i, src_i] = 1 for bound Node sources passing ALL source labels (:556-601)
    std::vector<u64> src_ids(k, ~0ull);
    std::vector<u64> cand_rows, cand_nodes;
    for (u64 i = 0; i < k; ++i) {
        if (src[i].kind != Value::Node) {
            if (optional) continue;
            return false;                                               // per-row fallback (:566-575)
        }
        cand_rows.push_back(i);
        cand_nodes.push_back(src[i].id);
    }
    std::vector<uint8_t> ok;
    nodes_have_labels(g, *src_lids, cand_nodes, ok);   // node_has_label_id for every (row, label), batched
    bool any = false;
    for (size_t c = 0; c < cand_rows.size(); ++c)
        if (ok[c]) { src_ids[cand_rows[c]] = cand_nodes[c]; any = true; }
    if (!any) return null_pad();

    std::vector<u64> bitmap;
    if (!last_dst->empty()) bitmap = g.label_bitmap(*last_dst);         // dst label filter of the LAST hop (:647-651)
    lap("source labels, bitmap");

    // The chain runs once on the device and BOTH result columns are built there (fgpu_expand_pairs): the source-row index of
    // every pair expanded from the row pointers, a row with a pre-bound `to` cut down to that one destination (:657-661) —
    // they arrive by DMA in pinned blocks the operator hands on as they are.  (Round 4 streamed the destinations and built the
    // row column on the host: 10.5 ms against 4.1 ms for the bare device call on a 16.6 M-pair batch.)
    fgpu_ctx* ctx = g.ctx().raw();
    u64 fl = 0, np = 0;
    std::vector<u64> pinned_to;
    if (to_bound) {
        bool any_pinned = false;
        pinned_to.assign(k, ~0ull);
        for (u64 i = 0; i < k; ++i)
            if ((*to_bound)[i].kind == Value::Node) { pinned_to[i] = (*to_bound)[i].id; any_pinned = true; }
        if (!any_pinned) pinned_to.clear();
    }
    const bool want_edge = bind_relationship && hops.size() == 1;
    bool all_pinned = !pinned_to.empty();
    for (u64 i = 0; i < k && all_pinned; ++i)
        if (src_ids[i] != ~0ull && pinned_to[i] == ~0ull) all_pinned = false;
    if (all_pinned) {
        // every row of the batch has its destination bound (the multi-hop ExpandInto shape, test_expand_into.py:63-95): the
        // last hop is one probe per row of the chain's state (fgpu_expand_probe) — nothing is expanded, emitted or copied
        std::vector<uint8_t> present(k, 0);
        check(fgpu_expand_probe(ctx, src_ids.data(), pinned_to.data(), k, hl.m.data(), hl.dp.data(), hl.dm.data(), (int)hops.size(),
                                bitmap.empty() ? nullptr : bitmap.data(), present.data(), &fl),
              "CondTraverse::expand_batch (pinned)");
        for (u64 i = 0; i < k; ++i)
            if (present[i] && src_ids[i] != ~0ull) { rows.active_row.push_back(i); rows.dest.push_back(pinned_to[i]); }
        if (flops) *flops = fl;
        lap("fgpu_expand_probe");
    } else {
    const int row_bits = k > 65536 ? 32 : 16;                // (more than 64 child batches coalesced into one call)
    rows.row_pin = EngineBuf<uint16_t>(ctx);
    rows.row_pin32 = EngineBuf<uint32_t>(ctx);
    rows.dest_pin = EngineBuf<uint32_t>(ctx);
    void** prow = row_bits == 16 ? (void**)rows.row_pin.out() : (void**)rows.row_pin32.out();
    check(fgpu_expand_pairs32(ctx, src_ids.data(), k, hl.m.data(), hl.dp.data(), hl.dm.data(), (int)hops.size(),
                              bitmap.empty() ? nullptr : bitmap.data(), pinned_to.empty() ? nullptr : pinned_to.data(), row_bits, prow,
                              rows.dest_pin.out(), &np, &fl),
          "CondTraverse::expand_batch");
    rows.n_pin = np;
    if (flops) *flops = fl;
    lap("fgpu_expand_pairs");
    }
    if (want_edge) {
        // representative edge: first id found scanning the types in order (:663-695), batched per type
        const std::vector<u64>& tids = type_ids[0];
        rows.materialize();                                          // (this path drops and annotates pairs in place)
        const size_t n = rows.dest.size();
        std::vector<u64> es(n);
        for (size_t r = 0; r < n; ++r) es[r] = src_ids[rows.active_row[r]];
        std::vector<std::optional<u64>> rep(n);
        for (u64 t : tids) {
            std::vector<std::vector<u64>> ids;
            if (transposed) g.relationship_tensors()[t].get_batch(rows.dest, es, ids);   // the stored pair is (reached, bound)
            else g.relationship_tensors()[t].get_batch(es, rows.dest, ids);
            for (size_t r = 0; r < n; ++r)
                if (!rep[r] && !ids[r].empty()) rep[r] = ids[r][0];
        }
        size_t o = 0;
        rows.edge.resize(n);
        for (size_t r = 0; r < n; ++r) {
            if (!rep[r]) continue;                                                   // no edge: the pair is dropped
            rows.active_row[o] = rows.active_row[r];
            rows.dest[o] = rows.dest[r];
            rows.edge[o] = *rep[r];
            ++o;
        }
        rows.active_row.resize(o);
        rows.dest.resize(o);
        rows.edge.resize(o);
    }
    return null_pad();
}

void ExpandedRows::materialize() {
    if (!pinned()) return;
    active_row.resize(n_pin);
    dest.resize(n_pin);
    for (size_t i = 0; i < n_pin; ++i) { active_row[i] = row_pin.p ? (u64)row_pin.p[i] : (u64)row_pin32.p[i]; dest[i] = dest_pin.p[i]; }
    release_pinned();
}

void CondTraverseOp::expand_row(const Graph& g, std::optional<u64> from_id, std::optional<u64> to_id, bool transposed,
                                const std::vector<u64>& used_edges, std::vector<std::array<u64, 3>>& out,
                                BidirDedup* dedup, std::optional<u64> dedup_src) const {
    const Hop& h = hops.at(0);
    // build_state (cond_traverse.rs:362-440): labels of the matrix source / destination for the forward pass and,
    // for a bidirectional pattern, for the reverse pass; any unknown label or an unresolvable type is no_match
    const std::vector<u64> scan = scanned_type_ids(g, h.types);          // edge_type_indices (:418-426)
    if (!h.types.empty() && scan.empty()) return;                        // no_match: build_unrestricted_iter -> None
    auto from_l = g.resolve_label_ids(src_labels);
    auto to_l = g.resolve_label_ids(h.dst_labels);
    if (!from_l || !to_l) return;
    const std::vector<LabelId>& fwd_src_l = transposed ? *to_l : *from_l;
    const std::vector<LabelId>& fwd_dst_l = transposed ? *from_l : *to_l;
    const std::vector<LabelId>& rev_src_l = transposed ? *from_l : *to_l;       // :376-389
    const std::vector<LabelId>& rev_dst_l = transposed ? *to_l : *from_l;

    // rows [lo, hi] of the unrestricted pair matrix in ascending (row, col) order (build_unrestricted_iter :196-209)
    auto fwd_rows = [&](u64 lo, u64 hi) {
        if (h.types.empty()) return g.adjacency_matrix().iter(lo, hi);
        if (h.types.size() == 1) return g.relationship_tensors()[scan[0]].structural_iter(lo, hi);
        return g.build_relationship_matrix_unrestricted(scan).iter(lo, hi);
    };
    // row d of the TRANSPOSED pair matrix: (dest, src) ascending (build_transposed_iter :221-235)
    auto bwd_row = [&](u64 d) {
        if (h.types.size() == 1) return g.relationship_tensors()[scan[0]].matrix_t().iter(d, d);
        Matrix a = h.types.empty() ? g.adjacency_matrix().extract() : g.build_relationship_matrix_unrestricted(scan);
        return a.transpose().iter(d, d);
    };
    // (src, dst) matrix coordinates of one pass (:852-874 / :897-921)
    auto pairs_of = [&](std::optional<u64> msrc, std::optional<u64> mdst, bool drop_loops) {
        std::vector<std::pair<u64, u64>> pairs;
        if (!msrc && mdst) {
            for (auto& e : bwd_row(*mdst)) pairs.push_back({e.col, e.row});
        } else {
            for (auto& e : fwd_rows(msrc ? *msrc : 0, msrc ? *msrc : ~0ull))
                if (!mdst || *mdst == e.col) pairs.push_back({e.row, e.col});
        }
        if (drop_loops)
            pairs.erase(std::remove_if(pairs.begin(), pairs.end(), [](auto& p) { return p.first == p.second; }), pairs.end());
        return pairs;
    };
    // process_pairs (:978-1117), without the attribute filters (the attribute store is out of scope)
    auto process = [&](const std::vector<std::pair<u64, u64>>& pairs, bool is_reverse, const std::vector<LabelId>& sl,
                       const std::vector<LabelId>& dl) {
        for (auto& pr : pairs) {
            const u64 s = pr.first, d = pr.second;
            bool okl = true;
            for (LabelId l : sl) okl = okl && g.node_has_label_id(s, l);
            for (LabelId l : dl) okl = okl && g.node_has_label_id(d, l);
            if (!okl) continue;
            const u64 from_node = is_reverse ? d : s, to_node = is_reverse ? s : d;
            if (from_id && *from_id != from_node) continue;
            if (to_id && *to_id != to_node) continue;
            const bool first_only = !emit_relationship;                  // one representative edge per pair (:1063-1081)
            bool done = false;
            for (u64 t : scan) {
                for (u64 id : g.relationship_tensors()[t].get(s, d)) {
                    if (std::find(used_edges.begin(), used_edges.end(), id) != used_edges.end()) continue;
                    out.push_back({from_node, to_node, id});
                    if (first_only) { done = true; break; }
                }
                if (done) break;
            }
        }
    };
    const size_t start = out.size();
    const std::optional<u64> fwd_src = transposed ? to_id : from_id, fwd_dst = transposed ? from_id : to_id;
    process(pairs_of(fwd_src, fwd_dst, false), transposed, fwd_src_l, fwd_dst_l);
    if (bidirectional) {                                                 // the reverse relationships (:894-945)
        const std::optional<u64> rev_src = transposed ? from_id : to_id, rev_dst = transposed ? to_id : from_id;
        process(pairs_of(rev_src, rev_dst, true), !transposed, rev_src_l, rev_dst_l);
    }
    // anonymous bidirectional CT over an anonymous bidirectional child: one row per (scan source, final dest) across the
    // expand_row calls of a batch — swap_remove, as the reference does, so the surviving order is the reference's (:948-970)
    if (dedup && dedup_src) {
        size_t i = start;
        while (i < out.size()) {
            if (!dedup->seen.insert({*dedup_src, out[i][1]}).second) {
                out[i] = out.back();
                out.pop_back();
                continue;
            }
            ++i;
        }
    }
}

bool CondTraverseOp::edges_batch_eligible(bool cross_row_dedup) const {
    return hops.size() == 1 && !has_inline_attrs && (emit_relationship || bidirectional || has_sibling_edges) && !cross_row_dedup;
}

bool CondTraverseOp::expand_batch_edges(const Graph& g, const std::vector<Value>& from, const std::vector<Value>& to, bool transposed,
                                        const u64* used, u64 n_used, EdgeRows& rows, std::vector<u64>& null_rows, u64* stats,
                                        bool cross_row_dedup) const {
    rows.clear();
    null_rows.clear();
    if (stats) std::fill(stats, stats + 8, 0);
    if (!edges_batch_eligible(cross_row_dedup)) return false;
    const u64 k = from.size();
    if (to.size() != k) throw GrbError(FGPU_INVALID, "expand_batch_edges: from and to differ in length");
    auto finish = [&]() {                                                // OPTIONAL: the rows without an emission
        if (optional) append_rows_without_emission(k, rows.size(), [&](size_t r) { return rows.row[r]; }, null_rows);
        return true;
    };
    const Hop& h = hops.at(0);
    // build_state (cond_traverse.rs:362-440), as expand_row: a single unknown type or an alternation of unknown names is
    // no_match, unknown names of an alternation are dropped, an unknown label is no_match.
    // No type named: every tensor, in id order (edge_type_indices, :418-426).  The reference walks the ADJACENCY there and the
    // device walks the union of the tensors' structures: the same pairs, by the Graph invariant that the adjacency is that union
    // (create_edge / delete_edge and the four bulk mutations write both sides together).
    const std::vector<u64> scan = scanned_type_ids(g, h.types);
    if (!h.types.empty() && scan.empty()) return finish();
    auto from_l = g.resolve_label_ids(src_labels);
    auto to_l = g.resolve_label_ids(h.dst_labels);
    if (!from_l || !to_l) return finish();

    // the rows: ~0 = unbound; a row bound to a non-node is skipped (:796-805), one with nothing bound is the host's
    std::vector<u64> f(k, ~0ull), t(k, ~0ull);
    std::vector<uint8_t> live(k, 0), full_walk(k, 0);
    bool all_from = true, all_to = true, any = false;
    for (u64 i = 0; i < k; ++i) {
        const Value::Kind fk = from[i].kind, tk = to[i].kind;
        if (fk == Value::Null || fk == Value::Other || tk == Value::Null || tk == Value::Other) continue;
        if (fk == Value::Unbound && tk == Value::Unbound) { full_walk[i] = 1; continue; }
        live[i] = 1;
        any = true;
        if (fk == Value::Node) f[i] = from[i].id; else all_from = false;
        if (tk == Value::Node) t[i] = to[i].id; else all_to = false;
    }
    // labels: from_node carries the source labels and to_node the destination labels in both passes (fgpu.h).  A side every live
    // row has bound is that row's from_node / to_node: probed here; otherwise the bitmap goes to the device
    std::vector<u64> from_bm, to_bm;
    auto side_labels = [&](const std::vector<LabelId>& lids, bool all_bound, std::vector<u64>& ids, std::vector<u64>& bm) {
        if (lids.empty() || !any) return;
        if (!all_bound) { bm = g.label_bitmap(lids); return; }
        std::vector<u64> idx, nodes;
        for (u64 i = 0; i < k; ++i)
            if (live[i]) { idx.push_back(i); nodes.push_back(ids[i]); }
        std::vector<uint8_t> ok;
        nodes_have_labels(g, lids, nodes, ok);
        for (size_t c = 0; c < idx.size(); ++c)
            if (!ok[c]) live[idx[c]] = 0;
    };
    side_labels(*from_l, all_from, f, from_bm);
    side_labels(*to_l, all_to, t, to_bm);
    for (u64 i = 0; i < k; ++i)
        if (!live[i]) f[i] = t[i] = ~0ull;                               // (the device skips a row with nothing bound)

    const TensorLayerArrays tl = gather(g, scan);                        // the layers of every scanned tensor
    const size_t T = tl.size();
    const bool filter = used && n_used;
    const bool first_only = !emit_relationship;
    const int flags = (transposed ? FGPU_EDGES_TRANSPOSED : 0) | (bidirectional ? FGPU_EDGES_BIDIRECTIONAL : 0) |
                      (first_only && !filter ? FGPU_EDGES_FIRST_ONLY : 0);
    fgpu_ctx* ctx = g.ctx().raw();
    EngineBuf<uint32_t> orow(ctx), ofrom(ctx), oto(ctx);
    EngineBuf<u64> oid(ctx);
    EngineBuf<uint8_t> opass(ctx);
    u64 n = 0;
    if (T && any)
        check(fgpu_expand_edges(ctx, f.data(), t.data(), k, tl.m.data(), tl.dp.data(), tl.dm.data(), tl.tm.data(), tl.tdp.data(),
                                tl.tdm.data(), tl.multi.data(), (int)T, flags, from_bm.empty() ? nullptr : from_bm.data(),
                                to_bm.empty() ? nullptr : to_bm.data(),
                                orow.out(), ofrom.out(), oto.out(), oid.out(), filter ? opass.out() : nullptr, &n, stats),
              "CondTraverse::expand_batch_edges");

    // the columns, the full-matrix rows spliced in at their place, the sibling-bound ids dropped
    size_t q = 0;
    auto device_rows_below = [&](u64 bound) {
        uint32_t g_row = ~0u, g_from = 0, g_to = 0;
        uint8_t g_pass = 0;
        bool g_done = false;
        for (; q < n && orow[q] < bound; ++q) {
            const u64 r = orow[q];
            if (filter) {
                if (orow[q] != g_row || ofrom[q] != g_from || oto[q] != g_to || opass[q] != g_pass) {
                    g_row = orow[q]; g_from = ofrom[q]; g_to = oto[q]; g_pass = opass[q];
                    g_done = false;
                }
                if (g_done) continue;
                const u64* u = used + r * n_used;
                if (std::find(u, u + n_used, oid[q]) != u + n_used) continue;
                if (first_only) g_done = true;
            }
            rows.push(r, ofrom[q], oto[q], oid[q]);
        }
    };
    for (u64 i = 0; i < k; ++i) {
        if (!full_walk[i]) continue;
        device_rows_below(i);
        std::vector<std::array<u64, 3>> out;
        const std::vector<u64> u(filter ? used + i * n_used : nullptr, filter ? used + (i + 1) * n_used : nullptr);
        expand_row(g, std::nullopt, std::nullopt, transposed, u, out);
        for (auto& x : out) rows.push(i, x[0], x[1], x[2]);
    }
    device_rows_below(k);
    return finish();
}

// ---- SemiApply / AntiSemiApply / OrApplyMultiplexer ---------------------------------------------------------------------
void SemiApplyOp::match_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to, bool transposed,
                              std::vector<uint8_t>& matched, Stats* stats) const {
    const u64 k = from.size();
    matched.assign(k, 0);
    Stats st;
    if (to && to->size() != k) throw GrbError(FGPU_INVALID, "SemiApply: from and to differ in length");
    // the rows that can emit at all: the bound alias is a node, and `to` is a node or unbound (:796-805)
    std::vector<u64> live;
    std::vector<Value> lf, lt;
    u64 n_bound = 0;
    for (u64 i = 0; i < k; ++i) {
        if (from[i].kind != Value::Node) continue;
        const Value t = to ? (*to)[i] : Value{};
        if (t.kind == Value::Null || t.kind == Value::Other) continue;
        live.push_back(i);
        lf.push_back(from[i]);
        lt.push_back(t);
        if (t.kind == Value::Node) ++n_bound;
    }
    const u64 n = live.size();
    auto done = [&]() { if (stats) *stats = st; };
    if (n == 0) return done();
    CondTraverseOp p = pattern;                  // the branch as this call runs it: never optional, in the caller's direction
    p.optional = false;
    p.transposed = transposed;
    const bool matrix = p.batched_eligible() && (!transposed || p.hops.size() == 1);
    const bool edges = p.edges_batch_eligible();
    fgpu_ctx* ctx = g.ctx().raw();

    // one fgpu_expand_exists over the layers of one direction: the bound node carries the source labels, the node it reaches
    // the last hop's; false = no_match (an unknown type or label: nothing can match)
    auto exists_over = [&](bool over_transposed, std::vector<uint64_t>& bits) {
        HopLayers hl;
        std::vector<std::vector<u64>> type_ids;
        if (!hop_layers(g, p.hops, hl, type_ids, over_transposed)) return false;
        auto last_dst = g.resolve_label_ids(p.hops.back().dst_labels);
        auto src_lids = g.resolve_label_ids(p.src_labels);
        if (!last_dst || !src_lids) return false;
        std::vector<u64> nodes(n), src_ids(n, ~0ull);
        for (u64 c = 0; c < n; ++c) nodes[c] = lf[c].id;
        std::vector<uint8_t> ok;
        nodes_have_labels(g, *src_lids, nodes, ok);
        bool any = false;
        for (u64 c = 0; c < n; ++c)
            if (ok[c]) { src_ids[c] = nodes[c]; any = true; }
        if (!any) return true;
        std::vector<u64> bitmap;
        if (!last_dst->empty()) bitmap = g.label_bitmap(*last_dst);
        std::vector<uint64_t> got((n + 63) / 64, 0);
        u64 ds[4] = {0, 0, 0, 0};
        check(fgpu_expand_exists(ctx, src_ids.data(), n, hl.m.data(), hl.dp.data(), hl.dm.data(), (int)p.hops.size(),
                                 bitmap.empty() ? nullptr : bitmap.data(), got.data(), nullptr, ds),
              "SemiApply::match_batch");
        for (size_t w = 0; w < got.size(); ++w) bits[w] |= got[w];
        ++st.calls;
        for (int j = 0; j < 3; ++j) st.device[j] += ds[j];
        st.device[3] = ds[3];
        return true;
    };
    auto from_bits = [&](const std::vector<uint64_t>& bits) {
        for (u64 c = 0; c < n; ++c)
            if ((bits[c >> 6] >> (c & 63)) & 1ull) matched[live[c]] = 1;
    };

    if (device_exists && matrix && n_bound == 0) {
        st.tier = Exists;
        std::vector<uint64_t> bits((n + 63) / 64, 0);
        exists_over(transposed, bits);
        from_bits(bits);
        return done();
    }
    if (device_exists && !matrix && edges && !p.emit_relationship && !p.has_sibling_edges && n_bound == 0) {
        st.tier = Exists;                        // bidirectional: either direction, the same label roles
        std::vector<uint64_t> bits((n + 63) / 64, 0);
        if (exists_over(false, bits)) exists_over(true, bits);
        from_bits(bits);
        return done();
    }
    if (matrix) {
        // every row bound: expand_batch answers with its probe, nothing expanded (the ExpandInto shape) — the existence
        // tier; otherwise the pairs, and the rows that occur
        st.tier = (device_exists && n_bound == n) ? Exists : Collect;
        ExpandedRows rows;
        std::vector<u64> nulls;
        if (p.expand_batch(g, lf, n_bound ? &lt : nullptr, rows, nulls)) {
            for (size_t r = 0; r < rows.size(); ++r) matched[live[rows.row_at(r)]] = 1;
            rows.release_pinned();
            return done();
        }
    } else if (edges) {
        st.tier = Collect;
        CondTraverseOp::EdgeRows rows;
        std::vector<u64> nulls;
        if (p.expand_batch_edges(g, lf, lt, transposed, nullptr, 0, rows, nulls)) {
            for (u64 r : rows.row) matched[live[r]] = 1;
            return done();
        }
    }
    st.tier = PerRow;
    if (p.hops.size() != 1) throw GrbError(FGPU_INVALID, "SemiApply: a fused chain that the batch path declines has no per-row form");
    for (u64 c = 0; c < n; ++c) {
        std::vector<std::array<u64, 3>> out;
        p.expand_row(g, lf[c].id, lt[c].kind == Value::Node ? std::optional<u64>(lt[c].id) : std::nullopt, transposed, {}, out);
        if (!out.empty()) matched[live[c]] = 1;
    }
    done();
}

void SemiApplyOp::filter_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to, bool transposed,
                               std::vector<u64>& passing, Stats* stats) const {
    std::vector<uint8_t> matched;
    match_batch(g, from, to, transposed, matched, stats);
    passing.clear();
    for (u64 i = 0; i < matched.size(); ++i)
        if ((matched[i] != 0) != anti) passing.push_back(i);
}

void OrApplyMultiplexerOp::filter_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to,
                                        std::vector<u64>& passing, std::vector<SemiApplyOp::Stats>* stats) const {
    const u64 k = from.size();
    std::vector<uint8_t> pass(k, 0), matched;
    if (stats) stats->assign(branches.size(), SemiApplyOp::Stats{});
    for (size_t b = 0; b < branches.size(); ++b) {
        const Branch& br = branches[b];
        if (br.semi) {
            br.semi->match_batch(g, from, to, br.transposed, matched, stats ? &(*stats)[b] : nullptr);
        } else {
            if (br.column.size() != k) throw GrbError(FGPU_INVALID, "OrApplyMultiplexer: a column branch needs one byte per row");
            matched = br.column;
        }
        for (u64 i = 0; i < k; ++i)
            if ((matched[i] != 0) != br.anti) pass[i] = 1;
    }
    passing.clear();
    for (u64 i = 0; i < k; ++i)
        if (pass[i]) passing.push_back(i);
}

// ---- CondVarLenTraverse ---------------------------------------------------------------------------------
namespace {
struct VlEdge { u64 src, dst, id; };

// Graph::get_node_relationships_by_type (graph.rs:1797-1835): per tensor (all of them, or the known ones among `types`,
// in order) the outgoing half — Tensor::iter(id, id, false): (dst, edge id) ascending — then the incoming half —
// Tensor::iter(id, id, true) over `mt`: (src, edge id) ascending — without the self-loops the outgoing half already gave
std::vector<VlEdge> node_relationships(const Graph& g, u64 id, const std::vector<u64>& tids, bool outgoing, bool incoming) {
    std::vector<VlEdge> out;
    for (u64 t : tids) {
        const Tensor& T = g.relationship_tensors()[t];
        if (outgoing)
            for (auto& e : T.structural_iter(id, id))
                for (u64 eid : T.get(e.row, e.col)) out.push_back({e.row, e.col, eid});
        if (incoming)
            for (auto& e : T.matrix_t().iter(id, id)) {          // row = dst (= id), col = src
                if (outgoing && e.col == id) continue;
                for (u64 eid : T.get(e.col, id)) out.push_back({e.col, id, eid});
            }
    }
    return out;
}

// What a CondVarLenTraverse walks and filters by, resolved once per row or batch.  Types: none named = every tensor; named =
// the known ones (filter_map, graph.rs:1803-1810) — with none known the walk is empty and the 0-hop rows still appear.
// Destination labels: an unknown one suppresses every emission (:100-107).
struct VarLenScan {
    std::vector<u64> tids;
    std::vector<LabelId> dl;
    bool label_missing = false;
    VarLenScan(const Graph& g, const CondVarLenTraverseOp& op) : tids(scanned_type_ids(g, op.types)) {
        for (auto& l : op.dst_labels) {
            if (auto id = g.label_id(l)) dl.push_back(*id);
            else label_missing = true;
        }
    }
};
}  // namespace

void CondVarLenTraverseOp::expand_row(const Graph& g, u64 start, std::optional<u64> dest, std::vector<VarLenRow>& out,
                                      VarLenStats* stats) const {
    VarLenStats local;
    VarLenStats& st = stats ? *stats : local;
    const VarLenScan scan(g, *this);
    auto labels_ok = [&](u64 v) {
        for (LabelId l : scan.dl)
            if (!g.node_has_label_id(v, l)) return false;
        return true;
    };
    const bool with_out = bidirectional || !reversed, with_in = bidirectional || reversed;
    auto emit = [&](u64 other, const std::vector<u64>& walk) {
        VarLenRow r;
        r.from = reversed ? other : start;
        r.to = reversed ? start : other;
        if (emit_path) {
            r.path = walk;
            if (reversed) std::reverse(r.path.begin(), r.path.end());   // path_value (:134-142)
        }
        out.push_back(std::move(r));
    };
    // 0-hop emission (:153-171)
    if (min_hops == 0 && (!dest || *dest == start) && !scan.label_missing && labels_ok(start)) emit(start, {start});

    // reach[r] (r >= 1): nodes from which `dest` is reachable by a walk of 1..r steps in the direction the DFS moves.
    // Walking back from dest: the DFS follows A (outgoing), A' (reversed) or A + A' (bidirectional), so the sets grow by
    // products with A', A or A + A'.  Only worth it for a bound destination and a finite budget.
    std::vector<std::vector<uint64_t>> reach;
    const u64 n = g.node_cap();
    if (prune && dest && max_hops != UINT32_MAX && max_hops >= 2 && max_hops <= 64 && !scan.tids.empty()) {
        // (build_adjacency_matrix takes the names: none = the adjacency of every type, unknown names are skipped)
        Matrix back = bidirectional ? g.build_symmetric_adjacency_matrix(types)
                                    : (reversed ? g.build_adjacency_matrix(types) : g.build_adjacency_matrix(types).transpose());
        Matrix f(g.ctx(), Type::Bool, 1, n);
        f.build({0}, {*dest});
        std::vector<uint64_t> acc((n + 63) / 64, 0);
        reach.resize(max_hops);                       // reach[r] for r in [1, max_hops - 1]
        for (uint32_t r = 1; r + 1 <= max_hops; ++r) {
            f.lmxm(back);
            ++st.reach_products;
            for (auto& e : f.iter(0, 0)) acc[e.col >> 6] |= 1ull << (e.col & 63);
            reach[r] = acc;
            if (f.nvals() == 0) {                     // the frontier died out: larger budgets add nothing
                for (uint32_t q = r + 1; q + 1 <= max_hops; ++q) reach[q] = acc;
                break;
            }
        }
    }
    auto can_reach = [&](u64 v, uint32_t budget) {
        if (reach.empty() || budget == 0) return true;
        if (budget >= reach.size()) budget = (uint32_t)reach.size() - 1;
        return ((reach[budget][v >> 6] >> (v & 63)) & 1ull) != 0;
    };

    struct Frame { u64 node; std::vector<u64> walk; std::vector<u64> used; uint32_t depth; };
    std::vector<Frame> stack;
    std::unordered_map<u64, std::vector<VlEdge>> adj_cache;          // per row, like the reference's (:115-116)
    stack.push_back({start, emit_path ? std::vector<u64>{start} : std::vector<u64>{}, {}, 0});
    std::vector<std::pair<u64, u64>> scratch;                        // (edge id, neighbour)
    while (!stack.empty()) {
        Frame fr = std::move(stack.back());
        stack.pop_back();
        const uint32_t hop = fr.depth + 1;
        if (hop > max_hops) continue;
        ++st.frames;
        auto it = adj_cache.find(fr.node);
        if (it == adj_cache.end()) it = adj_cache.emplace(fr.node, node_relationships(g, fr.node, scan.tids, with_out, with_in)).first;
        scratch.clear();
        for (const VlEdge& e : it->second) {
            if (std::find(fr.used.begin(), fr.used.end(), e.id) != fr.used.end()) continue;   // relationship uniqueness
            if (reversed) { if (e.dst == fr.node) scratch.push_back({e.id, e.src}); }
            else if (e.src == fr.node) scratch.push_back({e.id, e.dst});
            else if (bidirectional && e.dst == fr.node) scratch.push_back({e.id, e.src});
        }
        for (auto& [eid, nb] : scratch) {
            const bool will_emit = hop >= min_hops && (!dest || *dest == nb) && !scan.label_missing && labels_ok(nb);
            bool will_continue = hop < max_hops;
            if (will_continue && !can_reach(nb, max_hops - hop)) { will_continue = false; ++st.pruned; }
            if (!will_emit && !will_continue) continue;
            std::vector<u64> walk = fr.walk;
            if (emit_path) { walk.push_back(eid); walk.push_back(nb); }
            if (will_emit) emit(nb, walk);
            if (will_continue) {
                std::vector<u64> used = fr.used;
                used.push_back(eid);
                stack.push_back({nb, std::move(walk), std::move(used), hop});
            }
        }
    }
}

void CondVarLenTraverseOp::expand_batch(const Graph& g, const std::vector<u64>& starts, const std::vector<std::optional<u64>>& dests,
                                        std::vector<u64>& out_row, std::vector<VarLenRow>& out, VarLenStats* stats,
                                        u64* device_calls) const {
    out_row.clear();
    out.clear();
    VarLenStats local;
    VarLenStats& st = stats ? *stats : local;
    if (device_calls) *device_calls = 0;
    const u64 k = starts.size();
    if (!dests.empty() && dests.size() != k) throw GrbError(FGPU_INVALID, "CondVarLenTraverse::expand_batch: starts and dests differ in length");
    const VarLenScan scan(g, *this);                                     // types and labels as expand_row resolves them
    if (scan.label_missing) return;                                      // no emission (:100-107), so no device call either
    std::vector<u64> bitmap;
    if (!scan.dl.empty()) bitmap = g.label_bitmap(scan.dl);
    auto dest_of = [&](u64 i) { return dests.empty() ? std::optional<u64>() : dests[i]; };

    // the rows the device takes, and the layers of every walked tensor as they lie there
    const u64 cap = g.node_cap();
    auto sendable = [&](u64 v) { return v < cap && !g.is_node_deleted(v); };
    std::vector<u64> idx, ds, dd;
    for (u64 i = 0; i < k; ++i) {
        const auto d = dest_of(i);
        if (!sendable(starts[i]) || (d && !sendable(*d))) continue;
        idx.push_back(i);
        ds.push_back(starts[i]);
        dd.push_back(d ? *d : ~0ull);
    }
    const TensorLayerArrays tl = idx.empty() ? TensorLayerArrays() : gather(g, scan.tids);   // (no row to send: no layer waited on)
    fgpu_ctx* ctx = g.ctx().raw();
    const int flags = (reversed ? FGPU_TRAILS_REVERSED : 0) | (bidirectional ? FGPU_TRAILS_BIDIRECTIONAL : 0) |
                      (emit_path ? FGPU_TRAILS_PATHS : 0);

    // the device's answers, in the order of idx: one chunk per call that fitted, or per single row the host walked instead
    struct Chunk {
        size_t lo, hi;
        EngineBuf<uint32_t> row, from, to, hops, pnode;
        EngineBuf<u64> poff, pedge;
        u64 n = 0;
        std::vector<VarLenRow> host_rows;
        bool host = false;
    };
    std::vector<Chunk> chunks;
    std::vector<std::pair<size_t, size_t>> todo{{0, idx.size()}};        // a stack: the left half is answered first
    while (!todo.empty()) {
        const auto [lo, hi] = todo.back();
        todo.pop_back();
        if (lo == hi) continue;
        Chunk c;
        c.lo = lo; c.hi = hi;
        c.row = EngineBuf<uint32_t>(ctx); c.from = EngineBuf<uint32_t>(ctx); c.to = EngineBuf<uint32_t>(ctx);
        c.hops = EngineBuf<uint32_t>(ctx); c.pnode = EngineBuf<uint32_t>(ctx);
        c.poff = EngineBuf<u64>(ctx); c.pedge = EngineBuf<u64>(ctx);
        u64 dstats[8] = {0};
        if (device_calls) ++*device_calls;
        const fgpu_info info = fgpu_expand_trails(
            ctx, ds.data() + lo, dests.empty() ? nullptr : dd.data() + lo, hi - lo, tl.m.data(), tl.dp.data(), tl.dm.data(), tl.tm.data(),
            tl.tdp.data(), tl.tdm.data(), tl.multi.data(), (int)tl.size(), flags, min_hops, max_hops,
            bitmap.empty() ? nullptr : bitmap.data(), device_budget,
            c.row.out(), c.from.out(), c.to.out(), c.hops.out(), emit_path ? c.poff.out() : nullptr, emit_path ? c.pnode.out() : nullptr,
            emit_path ? c.pedge.out() : nullptr, &c.n, dstats);
        if (info == FGPU_INSUFFICIENT_SPACE) {
            if (hi - lo == 1) {
                c.host = true;
                expand_row(g, ds[lo], dest_of(idx[lo]), c.host_rows, &st);
                chunks.push_back(std::move(c));
            } else {
                const size_t mid = lo + (hi - lo) / 2;
                todo.push_back({mid, hi});
                todo.push_back({lo, mid});
            }
            continue;
        }
        check(info, "CondVarLenTraverse::expand_batch");
        st.frames += dstats[0];
        chunks.push_back(std::move(c));
    }

    // the rows in input order, the host's spliced in at their place
    u64 next = 0, total = 0;                                             // the first input row not yet written
    for (const Chunk& c : chunks) total += c.host ? c.host_rows.size() : c.n;
    out.reserve(total);
    out_row.reserve(total);
    auto host_rows_below = [&](u64 bound) {
        for (; next < bound; ++next) {
            const size_t before = out.size();                            // (a row between two device rows is the host's)
            expand_row(g, starts[next], dest_of(next), out, &st);
            out_row.insert(out_row.end(), out.size() - before, next);
        }
    };
    for (Chunk& c : chunks) {
        u64 q = 0;
        for (size_t x = c.lo; x < c.hi; ++x) {
            host_rows_below(idx[x]);
            next = idx[x] + 1;
            if (c.host) {
                out_row.insert(out_row.end(), c.host_rows.size(), idx[x]);
                for (auto& r : c.host_rows) out.push_back(std::move(r));
                continue;
            }
            for (; q < c.n && c.row[q] == x - c.lo; ++q) {
                VarLenRow r;
                r.from = c.from[q];
                r.to = c.to[q];
                if (emit_path) {
                    const u64 b = c.poff[q], h = c.poff[q + 1] - b;
                    r.path.reserve(2 * h + 1);
                    for (u64 j = 0; j < h; ++j) { r.path.push_back(c.pnode[b + q + j]); r.path.push_back(c.pedge[b + j]); }
                    r.path.push_back(c.pnode[b + q + h]);
                }
                out_row.push_back(idx[x]);
                out.push_back(std::move(r));
            }
        }
    }
    host_rows_below(k);
}

// ---- ExpandInto ---------------------------------------------------------------------------------------
std::vector<std::array<u64, 3>> ExpandIntoOp::expand_row(const Graph& g, u64 src, u64 dst,
                                                         const std::vector<u64>& used_edges) const {
    std::vector<std::array<u64, 3>> out;
    std::vector<std::pair<u64, u64>> pairs{{src, dst}};
    if (bidirectional && src != dst) pairs.push_back({dst, src});
    auto tids = scanned_type_ids(g, types);
    for (auto& pr : pairs) {
        size_t before = out.size();
        for (u64 t : tids)
            for (u64 e : g.relationship_tensors()[t].get(pr.first, pr.second)) {
                if (std::find(used_edges.begin(), used_edges.end(), e) != used_edges.end()) continue;
                out.push_back({pr.first, pr.second, e});
            }
        if (!emit_relationship && out.size() > before + 1) out.resize(before + 1);   // one representative per pair
    }
    return out;
}

void ExpandIntoOp::expand_batch(const Graph& g, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                                std::vector<std::vector<std::array<u64, 3>>>& out) const {
    const size_t k = srcs.size();
    out.assign(k, {});
    auto tids = scanned_type_ids(g, types);
    // probe list: (src, dst) of every row, then (dst, src) of the rows that also look backwards
    std::vector<u64> ps(srcs), pd(dsts);
    std::vector<size_t> back_row;
    if (bidirectional)
        for (size_t i = 0; i < k; ++i)
            if (srcs[i] != dsts[i]) { ps.push_back(dsts[i]); pd.push_back(srcs[i]); back_row.push_back(i); }
    std::vector<std::vector<std::vector<u64>>> per_type(tids.size());
    for (size_t t = 0; t < tids.size(); ++t) g.relationship_tensors()[tids[t]].get_batch(ps, pd, per_type[t]);
    auto emit = [&](size_t row, size_t probe) {
        size_t before = out[row].size();
        for (size_t t = 0; t < tids.size(); ++t)
            for (u64 e : per_type[t][probe]) out[row].push_back({ps[probe], pd[probe], e});
        if (!emit_relationship && out[row].size() > before + 1) out[row].resize(before + 1);
    };
    for (size_t i = 0; i < k; ++i) emit(i, i);
    for (size_t b = 0; b < back_row.size(); ++b) emit(back_row[b], k + b);
}

// ---- AllShortestPaths -----------------------------------------------------------------------------------
// What both entry points do once the device has answered: the predecessor lists of ONE query's DAG — the pairs [p0, p0 + k) of
// from / to, sorted by (from, to), with fwd[t][p] / bwd[t][p] the relationship ids of type t behind pair p and behind its reverse
// — rebuilt in the reference's order, then the LIFO backtrack.  (A batch passes slices of the arrays of all its rows.)
static std::vector<std::vector<u64>> asp_walk(const AllShortestPathsOp& op, size_t ntypes, u64 src, u64 dst, int64_t L, u64 limit,
                                              const std::vector<u64>& from, const std::vector<u64>& to, size_t p0, size_t k,
                                              const std::vector<std::vector<std::vector<u64>>>& fwd,
                                              const std::vector<std::vector<std::vector<u64>>>& bwd) {
    std::vector<std::vector<u64>> out;
    const bool cycle = src == dst, bidirectional = op.bidirectional;
    const size_t p1 = p0 + k;
    // the pairs are sorted by (from, to): the out-pairs of a vertex are one run
    std::unordered_map<u64, std::pair<size_t, size_t>> run;
    for (size_t i = p0; i < p1;) {
        size_t j = i;
        while (j < p1 && from[j] == from[i]) ++j;
        run[from[i]] = {i, j};
        i = j;
    }
    // predecessor lists in the reference's order (:143-262 restricted to the DAG; see the comment in host.hpp).  Node 0 is
    // src; the other DAG vertices get their node when first reached; in the cycle shape the closing pairs (u, src) lead
    // to a node of their own, the end of the cycle
    struct Pred { size_t prev; u64 edge; };
    std::vector<u64> vertex{src};
    std::vector<std::vector<Pred>> preds(1);
    std::unordered_map<u64, size_t> node_of;
    if (!cycle) node_of[src] = 0;
    std::vector<size_t> level{0}, next;
    for (int64_t d = 0; d < L; ++d) {
        next.clear();
        for (size_t cur : level) {
            const auto r = run.find(vertex[cur]);
            if (r == run.end()) continue;
            auto reach = [&](size_t pair, const std::vector<u64>& ids) {
                if (ids.empty()) return;
                auto [it, fresh] = node_of.try_emplace(to[pair], vertex.size());
                if (fresh) {
                    vertex.push_back(to[pair]);
                    preds.emplace_back();
                    next.push_back(it->second);
                }
                for (u64 e : ids) preds[it->second].push_back({cur, e});
            };
            for (size_t t = 0; t < ntypes; ++t) {
                for (size_t p = r->second.first; p < r->second.second; ++p) reach(p, fwd[t][p]);          // outgoing by (dst, id)
                if (bidirectional)
                    for (size_t p = r->second.first; p < r->second.second; ++p)
                        if (from[p] != to[p]) reach(p, bwd[t][p]);                                      // incoming by (src, id)
            }
        }
        level.swap(next);
    }
    const auto end = node_of.find(dst);
    if (end == node_of.end()) return out;
    // the LIFO backtrack (:275-299)
    std::vector<std::pair<size_t, std::vector<u64>>> stack;
    stack.push_back({end->second, {}});
    while (!stack.empty()) {
        auto [node, path] = std::move(stack.back());
        stack.pop_back();
        if (node == 0) {
            if (!cycle) std::reverse(path.begin(), path.end());
            if (op.reversed) std::reverse(path.begin(), path.end());
            out.push_back(std::move(path));
            if (limit && out.size() >= limit) break;
            continue;
        }
        for (const Pred& p : preds[node]) {
            std::vector<u64> longer = path;
            longer.push_back(p.edge);
            stack.push_back({p.prev, std::move(longer)});
        }
    }
    return out;
}

std::vector<std::vector<u64>> AllShortestPathsOp::expand_row(const Graph& g, u64 src, u64 dst, u64 limit, int64_t* length) const {
    std::vector<std::vector<u64>> out;
    if (length) *length = -1;
    const u64 n = g.node_cap();
    if (src >= n || dst >= n || g.is_node_deleted(src) || g.is_node_deleted(dst)) return out;
    const std::vector<u64> tids = scanned_type_ids(g, types);            // (a name listed twice is walked twice: filter_map)
    if (tids.empty()) return out;
    Matrix adj = bidirectional ? g.build_symmetric_adjacency_matrix(types) : g.build_adjacency_matrix(types);
    Matrix adj_t = bidirectional ? adj : adj.transpose();
    int64_t L = -1;
    u64 k = 0;
    EdgeList dag(g.ctx());                                               // (rows, cols, vals) = (from, to, depth)
    check(fgpu_shortest_dag(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), src, dst, max_hops == UINT32_MAX ? -1 : (int64_t)max_hops,
                            &L, &k, dag.rows.out(), dag.cols.out(), (uint64_t**)dag.vals.out(), nullptr),
          "allShortestPaths");
    dag.n = k;
    if (L < 0) return out;
    if (length) *length = L;
    // the relationships behind every pair, per type: (u, v), and (v, u) under a bidirectional pattern
    const std::vector<u64> from(dag.rows.p, dag.rows.p + k), to(dag.cols.p, dag.cols.p + k);
    std::vector<std::vector<std::vector<u64>>> fwd(tids.size()), bwd(tids.size());
    for (size_t t = 0; t < tids.size(); ++t) {
        g.relationship_tensors()[tids[t]].get_batch(from, to, fwd[t]);
        if (bidirectional) g.relationship_tensors()[tids[t]].get_batch(to, from, bwd[t]);
    }
    return asp_walk(*this, tids.size(), src, dst, L, limit, from, to, 0, k, fwd, bwd);
}

std::vector<std::vector<std::vector<u64>>> AllShortestPathsOp::expand_batch(const Graph& g, const std::vector<u64>& srcs,
                                                                            const std::vector<u64>& dsts, u64 limit,
                                                                            std::vector<int64_t>* lengths, u64* device_calls) const {
    if (srcs.size() != dsts.size()) throw std::invalid_argument("allShortestPaths: srcs and dsts differ in length");
    const size_t count = srcs.size();
    std::vector<std::vector<std::vector<u64>>> out(count);
    if (lengths) lengths->assign(count, -1);
    if (device_calls) *device_calls = 0;
    const u64 n = g.node_cap();
    const std::vector<u64> tids = scanned_type_ids(g, types);
    if (tids.empty()) return out;
    // the rows the device sees: both nodes in range and alive
    std::vector<size_t> row;
    std::vector<u64> s, d;
    for (size_t i = 0; i < count; ++i) {
        if (srcs[i] >= n || dsts[i] >= n || g.is_node_deleted(srcs[i]) || g.is_node_deleted(dsts[i])) continue;
        row.push_back(i);
        s.push_back(srcs[i]);
        d.push_back(dsts[i]);
    }
    if (row.empty()) return out;
    // the pattern matrix and its transpose, once for the batch
    Matrix adj = bidirectional ? g.build_symmetric_adjacency_matrix(types) : g.build_adjacency_matrix(types);
    Matrix adj_t = bidirectional ? adj : adj.transpose();
    std::vector<int64_t> L(row.size(), -1);
    std::vector<u64> off(row.size() + 1, 0);
    EdgeList dag(g.ctx());                                               // (rows, cols, vals) = (from, to, depth) of every row
    check(fgpu_shortest_dag_batch(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), s.data(), d.data(), row.size(),
                                  max_hops == UINT32_MAX ? -1 : (int64_t)max_hops, 0, L.data(), off.data(), dag.rows.out(), dag.cols.out(),
                                  (uint64_t**)dag.vals.out(), nullptr),
          "allShortestPaths");
    if (device_calls) *device_calls = 1;
    const size_t k = off.back();
    dag.n = k;
    // the relationships behind the pairs of ALL rows: one probe per type and direction
    const std::vector<u64> from(dag.rows.p, dag.rows.p + k), to(dag.cols.p, dag.cols.p + k);
    std::vector<std::vector<std::vector<u64>>> fwd(tids.size()), bwd(tids.size());
    if (k)
        for (size_t t = 0; t < tids.size(); ++t) {
            g.relationship_tensors()[tids[t]].get_batch(from, to, fwd[t]);
            if (bidirectional) g.relationship_tensors()[tids[t]].get_batch(to, from, bwd[t]);
        }
    for (size_t j = 0; j < row.size(); ++j) {
        if (L[j] < 0) continue;
        if (lengths) (*lengths)[row[j]] = L[j];
        out[row[j]] = asp_walk(*this, tids.size(), s[j], d[j], L[j], limit, from, to, off[j], off[j + 1] - off[j], fwd, bwd);
    }
    return out;
}

// ---- shortestPath() ---------------------------------------------------------------------------------------
namespace {
// NeighborIter (eval.rs:140-244): the row of `node` in every matrix of the set, one sorted stream per matrix (the layers merged
// by the versioned iterators); several streams are sorted together and deduplicated (:238-241)
struct SpNeighbors {
    std::vector<const VersionedMatrix*> plain;   // iter()
    std::vector<const Tensor*> structural;       // structural_iter()
    std::vector<u64> operator()(u64 node) const {
        std::vector<u64> buf;
        for (const Tensor* t : structural)
            if (node < t->nrows())
                for (const Entry& e : t->structural_iter(node, node)) buf.push_back(e.col);
        for (const VersionedMatrix* m : plain)
            if (node < m->nrows())
                for (const Entry& e : m->iter(node, node)) buf.push_back(e.col);
        if (plain.size() + structural.size() > 1) {
            std::sort(buf.begin(), buf.end());
            buf.erase(std::unique(buf.begin(), buf.end()), buf.end());
        }
        return buf;
    }
};

// NeighborIter::new (:153-187) and new_reversed (:193-217).  Names of which none exists leave the set empty: no neighbour
SpNeighbors sp_neighbors(const Graph& g, const std::vector<std::string>& types, bool directed, bool reversed) {
    SpNeighbors nb;
    const std::vector<u64> tids = scanned_type_ids(g, types);
    if (reversed) {
        for (u64 t : tids) nb.plain.push_back(&g.relationship_tensors()[t].matrix_t());
        return nb;
    }
    if (types.empty()) {
        nb.plain.push_back(&g.adjacency_matrix());
    } else {
        for (u64 t : tids) nb.structural.push_back(&g.relationship_tensors()[t]);
    }
    if (!directed)
        for (u64 t : tids) nb.plain.push_back(&g.relationship_tensors()[t].matrix_t());
    return nb;
}

// the first relationship from u to v over the types in order, else the first from v to u (eval.rs:1502-1505)
template <class Ids>
void sp_first_edge(const Ids& forward, const Ids& backward, std::vector<u64>& edges) {
    for (const Ids* side : {&forward, &backward})
        for (const auto& ids : *side)
            if (!ids->empty()) { edges.push_back(ids->front()); return; }
}
}  // namespace

ShortestPathFn::Path ShortestPathFn::eval_row(const Graph& g, const Value& src_val, const Value& dst_val) const {
    Path out;
    for (const Value* v : {&src_val, &dst_val}) {   // (:1314-1323: the source is looked at first)
        if (v->kind == Value::Null) return out;
        if (v->kind != Value::Node) throw GrbError(FGPU_INVALID, "A shortestPath requires bound nodes");
    }
    const u64 src = src_val.id, dst = dst_val.id;
    if (min_hops == 0 && src == dst) {              // :1329-1332
        out.null = false;
        out.nodes.push_back(src);
        return out;
    }
    if (src == dst) return out;                     // :1406-1408
    const SpNeighbors nbrs[2] = {sp_neighbors(g, types, directed, false), sp_neighbors(g, types, directed, directed)};
    // bfs_shortest_path (:1410-1471): (parent, depth) per visited node
    std::unordered_map<u64, std::pair<u64, u64>> ball[2];
    ball[0][src] = {src, 0};
    ball[1][dst] = {dst, 0};
    std::vector<u64> front[2] = {{src}, {dst}}, next;
    u64 depth[2] = {0, 0};
    const u64 max_level = max_hops == UINT32_MAX ? ~0ull : (u64)max_hops;
    bool met = false;
    u64 best_od = 0, meet = 0;
    while (!met) {
        if (front[0].empty() || front[1].empty() || depth[0] + depth[1] >= max_level) return out;
        const int s = front[0].size() <= front[1].size() ? 0 : 1;
        next.clear();
        for (u64 cur : front[s])
            for (u64 nb : nbrs[s](cur)) {
                if (ball[s].count(nb)) continue;
                ball[s][nb] = {cur, depth[s] + 1};
                const auto o = ball[s ^ 1].find(nb);
                if (o == ball[s ^ 1].end()) { next.push_back(nb); continue; }
                if (!met || o->second.second < best_od) { met = true; best_od = o->second.second; meet = nb; }
            }
        front[s].swap(next);
        ++depth[s];
    }
    std::vector<u64> nodes{meet};                   // :1475-1488
    while (nodes.back() != src) nodes.push_back(ball[0].at(nodes.back()).first);
    std::reverse(nodes.begin(), nodes.end());
    while (nodes.back() != dst) nodes.push_back(ball[1].at(nodes.back()).first);
    if (nodes.size() - 1 < min_hops) return out;    // :1491-1493
    const std::vector<u64> tids = scanned_type_ids(g, types);
    for (size_t i = 0; i + 1 < nodes.size(); ++i) {
        std::vector<std::vector<u64>> fwd, bwd;
        for (u64 t : tids) {
            fwd.push_back(g.relationship_tensors()[t].get(nodes[i], nodes[i + 1]));
            bwd.push_back(g.relationship_tensors()[t].get(nodes[i + 1], nodes[i]));
        }
        std::vector<const std::vector<u64>*> f, b;
        for (size_t t = 0; t < tids.size(); ++t) { f.push_back(&fwd[t]); b.push_back(&bwd[t]); }
        sp_first_edge(f, b, out.edges);
    }
    out.null = false;
    out.nodes = std::move(nodes);
    return out;
}

std::vector<ShortestPathFn::Path> ShortestPathFn::eval_batch(const Graph& g, const std::vector<Value>& srcs,
                                                             const std::vector<Value>& dsts, u64* device_calls) const {
    if (srcs.size() != dsts.size()) throw std::invalid_argument("shortestPath: srcs and dsts differ in length");
    const size_t count = srcs.size();
    std::vector<Path> out(count);
    if (device_calls) *device_calls = 0;
    const u64 n = g.node_cap();
    const std::vector<u64> tids = scanned_type_ids(g, types);
    // the rows the device sees: two nodes in range and alive, src != dst, and a pattern with a type behind it.  The others
    // are eval_row's, in place (a non-node endpoint throws there, as it does per row)
    std::vector<size_t> row;
    std::vector<u64> s, d;
    for (size_t i = 0; i < count; ++i) {
        const Value &a = srcs[i], &b = dsts[i];
        if (!tids.empty() && a.kind == Value::Node && b.kind == Value::Node && a.id != b.id && a.id < n && b.id < n &&
            !g.is_node_deleted(a.id) && !g.is_node_deleted(b.id)) {
            row.push_back(i);
            s.push_back(a.id);
            d.push_back(b.id);
        } else {
            out[i] = eval_row(g, a, b);
        }
    }
    if (row.empty()) return out;
    // F and B (the table in include/fgpu.h), once for the batch
    Matrix f = directed ? g.build_adjacency_matrix(types) : g.build_symmetric_adjacency_matrix(types);
    Matrix b = directed ? f.transpose() : f;
    std::vector<int64_t> L(row.size(), -1);
    std::vector<u64> off(row.size() + 1, 0);
    EngineBuf<u64> nodes(g.ctx().raw());
    check(fgpu_shortest_path_batch(g.ctx().raw(), f.snapshot(), b.snapshot(), s.data(), d.data(), row.size(),
                                   max_hops == UINT32_MAX ? -1 : (int64_t)max_hops, 0, L.data(), off.data(), nodes.out(), nullptr),
          "shortestPath");
    if (device_calls) *device_calls = 1;
    // the relationships behind the consecutive pairs of ALL rows: one probe per type and direction
    std::vector<u64> pu, pv;
    for (size_t j = 0; j < row.size(); ++j)
        for (u64 k = off[j]; k + 1 < off[j + 1]; ++k) { pu.push_back(nodes[k]); pv.push_back(nodes[k + 1]); }
    std::vector<std::vector<std::vector<u64>>> fwd(tids.size()), bwd(tids.size());
    if (!pu.empty())
        for (size_t t = 0; t < tids.size(); ++t) {
            g.relationship_tensors()[tids[t]].get_batch(pu, pv, fwd[t]);
            g.relationship_tensors()[tids[t]].get_batch(pv, pu, bwd[t]);
        }
    size_t pair = 0;
    for (size_t j = 0; j < row.size(); ++j) {
        if (L[j] < 0) continue;
        Path& p = out[row[j]];
        p.nodes.assign(nodes.p + off[j], nodes.p + off[j + 1]);
        std::vector<const std::vector<u64>*> fw(tids.size()), bw(tids.size());
        for (int64_t e = 0; e < L[j]; ++e, ++pair) {
            for (size_t t = 0; t < tids.size(); ++t) { fw[t] = &fwd[t][pair]; bw[t] = &bwd[t][pair]; }
            sp_first_edge(fw, bw, p.edges);
        }
        p.null = (u64)L[j] < min_hops;   // (never: a found path has an edge and min_hops is 0 or 1)
        if (p.null) { p.nodes.clear(); p.edges.clear(); }
    }
    return out;
}

// ---- indegree() / outdegree() ----------------------------------------------------------------------------
namespace {
// parse_degree_args + get_node_*degree_by_type: none named = every tensor, else the known names, each once, in the order of
// their first mention
std::vector<u64> degree_type_ids(const Graph& g, const std::vector<std::string>& names) {
    if (names.empty()) return scanned_type_ids(g, names);
    std::vector<u64> ids;
    for (u64 id : named_type_ids(g, names))
        if (std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
    return ids;
}
void require_node_ids(const Graph& g, const std::vector<u64>& ids, const char* who) {
    for (u64 id : ids)
        if (id >= g.node_cap())
            throw std::out_of_range(std::string(who) + ": node id " + std::to_string(id) + " is at or past the node capacity " +
                                    std::to_string(g.node_cap()));
}
// ids == nullptr: the whole-graph form, k = node_cap()
std::vector<u64> device_degrees(const Graph& g, const std::vector<u64>& tids, bool incoming, const u64* ids, u64 k, u64* device_calls) {
    std::vector<u64> out(k, 0), part(k);
    if (device_calls) *device_calls = 0;
    if (k == 0) return out;
    for (size_t t0 = 0; t0 < tids.size(); t0 += 64) {
        const std::vector<u64> group(tids.begin() + t0, tids.begin() + std::min(tids.size(), t0 + 64));
        TensorLayerArrays a;
        if (incoming) {
            a = gather(g, group);
        } else {   // outgoing: the transposed layers are not read, so a pending transpose is not materialised
            for (u64 t : group) {
                const Tensor& ten = g.relationship_tensors()[t];
                ten.wait_fwd();
                const Layers f = fwd_layers(ten);
                a.m.push_back(f.m); a.dp.push_back(f.dp); a.dm.push_back(f.dm);
                a.multi.push_back(ten.multi_table());
            }
        }
        check(fgpu_node_degrees(g.ctx().raw(), ids, k, a.m.data(), a.dp.data(), a.dm.data(), incoming ? a.tm.data() : nullptr,
                                incoming ? a.tdp.data() : nullptr, incoming ? a.tdm.data() : nullptr, a.multi.data(), (int)a.size(),
                                incoming ? FGPU_DEGREE_IN : FGPU_DEGREE_OUT, incoming ? nullptr : part.data(),
                                incoming ? part.data() : nullptr, nullptr),
              incoming ? "indegree" : "outdegree");
        if (device_calls) ++*device_calls;
        for (u64 i = 0; i < k; ++i) out[i] += part[i];
    }
    return out;
}
}  // namespace

u64 DegreeFn::eval_row(const Graph& g, u64 id) const {
    require_node_ids(g, {id}, incoming ? "indegree" : "outdegree");
    return node_relationships(g, id, degree_type_ids(g, types), !incoming, incoming).size();
}

std::vector<u64> DegreeFn::eval_batch(const Graph& g, const std::vector<u64>& ids, u64* device_calls) const {
    require_node_ids(g, ids, incoming ? "indegree" : "outdegree");
    return device_degrees(g, degree_type_ids(g, types), incoming, ids.data(), ids.size(), device_calls);
}

std::vector<u64> DegreeFn::eval_all(const Graph& g, u64* device_calls) const {
    return device_degrees(g, degree_type_ids(g, types), incoming, nullptr, g.node_cap(), device_calls);
}

// ---- algo.BFS --------------------------------------------------------------------------------------------
// The partitioned form of the search below: the adjacency is cut into nnz-balanced column slabs, one
// per context of `gang` (one context per GPU; several contexts on one device work too and are how this is tested),
// and ONE call — fgpu_bfs_dist_run — drives every rank's level kernels and the per-level frontier exchange inside
// libfgpu.so (RCCL when the contexts were joined by fgpu_comm_init_all, event-ordered peer copies otherwise).
// Everything goes through include/fgpu.h.  Slabs that live on another context travel through the host once per
// call (no cross-device snapshot copy in the ABI yet; a cache keyed on the adjacency snapshot is the obvious next step).
static void bfs_partitioned(const Graph& g, const std::vector<Context*>& gang, const Matrix& adj, const std::string& key,
                            u64 source, int64_t max_depth, bool want_edges, std::vector<int32_t>& level,
                            std::vector<int64_t>& parent) {
    const int nr = (int)gang.size();
    fgpu_ctx* c0 = g.ctx().raw();
    std::vector<fgpu_ctx*> raw(nr);
    for (int r = 0; r < nr; ++r) raw[r] = gang[r]->raw();
    std::shared_ptr<Graph::BfsGangCache> gc = g.bfs_gang_cache_;
    if (!gc || gc->key != key || gc->gang != raw || gc->plans.empty() || gc->adj.snapshot() != adj.snapshot()) {
        // a new adjacency, filter or gang: cut the slabs again (the previous set is released with its last user)
        gc = std::make_shared<Graph::BfsGangCache>(adj);
        gc->key = key;
        gc->gang = raw;
        gc->splits.assign((size_t)nr + 1, 0);
        gc->slabs.resize(nr);
        gc->slabs_t.resize(nr);
        gc->plans.resize(nr);
        check(fgpu_mat_balanced_splits(c0, adj.snapshot(), nr, gc->splits.data()), "fgpu_mat_balanced_splits");
        const u64 n = g.node_cap();
        for (int r = 0; r < nr; ++r) {
            fgpu_ctx* cr = raw[r];
            SnapshotRef local;
            check(fgpu_mat_col_slab(c0, local.out(), adj.snapshot(), gc->splits[r], gc->splits[r + 1] < n ? gc->splits[r + 1] : n),
                  "fgpu_mat_col_slab");
            if (cr == c0) {
                gc->slabs[r] = std::move(local);
            } else {
                EngineBuf<u64> rp(c0), ci(c0);
                u64 nnz = 0;
                check(fgpu_mat_export_csr(c0, local.get(), rp.out(), ci.out(), nullptr, &nnz), "GxB_unload_Matrix_into_Container");
                local.reset();   // (the host arrays are all that travels: c0's copy goes before cr's is built)
                check(fgpu_mat_from_csr(cr, gc->slabs[r].out(), n, n, nnz, rp.p, 64, ci.p, 64, nullptr, nullptr, 0),
                      "GxB_load_Matrix_from_Container");
            }
            check(fgpu_mat_transpose(cr, gc->slabs_t[r].out(), gc->slabs[r].get()), "GrB_transpose");
            check(fgpu_bfs_plan_create_slab(cr, gc->plans[r].out(), gc->slabs[r].get(), gc->slabs_t[r].get(), r, nr, gc->splits.data()),
                  "fgpu_bfs_plan_create_slab");
        }
        g.bfs_gang_cache_ = gc;            // (an exception above leaves the old cache in place; gc frees what it built)
        Graph::register_gang_cache(gc);
    }
    std::vector<fgpu_bfs_plan*> plans(nr);
    for (int r = 0; r < nr; ++r) plans[r] = gc->plans[r].get();
    check(fgpu_bfs_dist_run(plans.data(), nr, source, max_depth < 0 ? -1 : max_depth, want_edges ? 1 : 0),
          "LAGr_BreadthFirstSearch (partitioned)");
    for (int r = 0; r < nr; ++r)   // every rank fills its own range [splits[r], splits[r+1])
        check(fgpu_bfs_fetch(plans[r], level.data(), want_edges ? parent.data() : nullptr), "fgpu_bfs_fetch");
}

BfsResult algo_bfs(const Graph& g, std::optional<u64> source, int64_t max_depth,
                   const std::optional<std::string>& rel_type, bool want_edges, const std::vector<Context*>* gang) {
    BfsResult res;
    const u64 n = g.node_cap();
    if (!source) return res;                                             // NULL source: no row (:1029)
    // node_count() == 0 is tested BEFORE the deleted-source check (:1043-1048): with every node deleted the reference
    // returns the empty batch, not "Source node not found"
    const u64 live = n > g.deleted_nodes_count() ? n - g.deleted_nodes_count() : 0;
    if (live == 0) return res;
    if (g.is_node_deleted(*source)) throw GrbError(FGPU_INVALID, "Source node not found in graph");
    std::vector<std::string> types;
    if (rel_type) types.push_back(*rel_type);
    Matrix adj = g.build_adjacency_matrix(types);                        // graph.rs:3870-3894
    const std::string key = rel_type ? *rel_type : std::string();
    std::vector<int32_t> level_v;
    std::vector<int64_t> parent_v;
    const int32_t* level = nullptr;                    // what the result loop reads: the vectors, or the plan cache's pinned blocks
    const int64_t* parent = nullptr;
    const bool partitioned = gang && gang->size() > 1 && adj.nvals() > 0;
    if (partitioned) {
        level_v.resize(n);
        parent_v.resize(want_edges ? n : 0);
        bfs_partitioned(g, *gang, adj, key, *source, max_depth, want_edges, level_v, parent_v);
        level = level_v.data(); parent = parent_v.data();
    }
    std::shared_ptr<Graph::BfsPlanCache> pc;
    std::unique_lock<std::mutex> run_lock;                 // held across run, fetch AND the result loop (it reads the entry's pinned blocks)
    if (!partitioned) {
        std::lock_guard<std::mutex> cache_guard(g.bfs_cache_mu_);
        pc = g.bfs_cache_;
        if (!pc || pc->key != key || pc->adj.snapshot() != adj.snapshot()) {
            // a new adjacency (the layers changed, or another type): new plan; a clean committed graph keeps handing
            // out the same snapshot (VersionedMatrix::extract shares the base) and its cached transpose
            pc = std::make_shared<Graph::BfsPlanCache>(adj, adj.transpose(), g.ctx().raw());
            pc->key = key;
            // plans index dense row pointers: a hypersparse adjacency (an unknown type's empty matrix, a tiny delta-only
            // graph) goes through the one-shot entry point below, which densifies it
            if (fgpu_bfs_plan_create(g.ctx().raw(), pc->plan.out(), pc->adj.snapshot(), pc->adj_t.snapshot(), 0, 1) != FGPU_OK)
                pc.reset();
            g.bfs_cache_ = pc;
        }
        if (pc) {
            run_lock = std::unique_lock<std::mutex>(pc->mu, std::try_to_lock);
            if (!run_lock.owns_lock()) pc.reset();         // another thread is searching on it: the one-shot path below
        }
    }
    if (partitioned) {
        // levels / parents were assembled from the ranks above
    } else if (pc) {
        if (pc->pin_rows < n) {                                          // (a new cache entry, or the node capacity grew)
            pc->parent_pin.reset();
            pc->pin_rows = 0;
            pc->level_pin.alloc(n, "fgpu_host_alloc");                   // (the old block goes first)
            pc->pin_rows = n;
        }
        if (want_edges && !pc->parent_pin.p) pc->parent_pin.alloc(pc->pin_rows, "fgpu_host_alloc");
        check(fgpu_bfs_run(pc->plan.get(), *source, max_depth < 0 ? -1 : max_depth, want_edges ? 1 : 0), "LAGr_BreadthFirstSearch");
        check(fgpu_bfs_fetch(pc->plan.get(), pc->level_pin.p, want_edges ? pc->parent_pin.p : nullptr), "LAGr_BreadthFirstSearch");
        level = pc->level_pin.p; parent = pc->parent_pin.p;
    } else {
        level_v.resize(n);
        parent_v.resize(want_edges ? n : 0);
        Matrix adj_t = adj.transpose();
        check(fgpu_bfs(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), *source, max_depth < 0 ? -1 : max_depth,
                       level_v.data(), want_edges ? parent_v.data() : nullptr, nullptr),
              "LAGr_BreadthFirstSearch");
        level = level_v.data(); parent = parent_v.data();
    }
    std::vector<u64> ps, pd;
    for (u64 v = 0; v < n; ++v) {
        if (level[v] < 0 || v == *source || g.is_node_deleted(v)) continue;
        if (want_edges) {
            u64 p = (u64)parent[v];
            if (g.is_node_deleted(p)) continue;
            ps.push_back(p);
            pd.push_back(v);
        }
        res.nodes.push_back(v);
    }
    if (want_edges && !res.nodes.empty()) {
        // edges[k] = first id of get_src_dest_relationships(parent, child, types), batched per type
        const std::vector<u64> tids = scanned_type_ids(g, types);
        std::vector<std::optional<u64>> rep(ps.size());
        for (u64 t : tids) {
            std::vector<std::vector<u64>> ids;
            g.relationship_tensors()[t].get_batch(ps, pd, ids);
            for (size_t r = 0; r < ps.size(); ++r)
                if (!rep[r] && !ids[r].empty()) rep[r] = ids[r][0];
        }
        for (auto& e : rep)
            if (e) res.edges.push_back(*e);
    }
    res.has_row = !res.nodes.empty();
    return res;
}

// ---- what algo.pageRank, algo.WCC and algo.betweenness share ---------------------------------------------
// The nodes a procedure runs over: the union of the labels' nodes minus the deleted ids (collect_node_ids, :456-477), as a
// bitmap over the full id space — the reference's compact graph (build_compact_adj_from_tensors), here an induced subgraph.
// An unknown label selects no node.  `ids` (nullable) receives the selected ids in ascending order (compact_to_id).
struct NodeSelection {
    std::vector<u64> bits;
    u64 count = 0;
    bool has(u64 v) const { return (bits[v >> 6] >> (v & 63)) & 1ull; }
};
static NodeSelection select_nodes(const Graph& g, const std::vector<std::string>& labels, std::vector<u64>* ids = nullptr) {
    const u64 n = g.node_cap();
    NodeSelection sel;
    sel.bits.assign((n + 63) / 64, 0);
    for (auto& l : labels)
        if (auto lid = g.label_id(l)) {
            const std::vector<u64> bits = g.label_bitmap({*lid});
            for (size_t w = 0; w < sel.bits.size(); ++w) sel.bits[w] |= bits[w];
        }
    for (u64 v = 0; v < n; ++v) {
        if (g.is_node_deleted(v)) sel.bits[v >> 6] &= ~(1ull << (v & 63));
        if (!sel.has(v)) continue;
        ++sel.count;
        if (ids) ids->push_back(v);
    }
    return sel;
}
// ... every live node (a procedure called without labels whose engine call wants the bitmap all the same)
static NodeSelection select_live_nodes(const Graph& g) {
    const u64 n = g.node_cap();
    NodeSelection sel;
    sel.bits.assign((n + 63) / 64, 0);
    for (u64 v = 0; v < n; ++v)
        if (!g.is_node_deleted(v)) { sel.bits[v >> 6] |= 1ull << (v & 63); ++sel.count; }
    return sel;
}
// rank[v] = v's index among the selected ids in ascending order (the reference's compact index), -1 for the others
static std::vector<int64_t> compact_ranks(const NodeSelection& sel, u64 n) {
    std::vector<int64_t> rank(n, -1);
    int64_t k = 0;
    for (u64 v = 0; v < n; ++v)
        if (sel.has(v)) rank[v] = k++;
    return rank;
}

// one result row per live node (sel, nullable: that is also selected), in id order; value(v) is the row's second column
template <typename T, typename F>
static void emit_rows(const Graph& g, const NodeSelection* sel, std::vector<u64>& nodes, std::vector<T>& values, F value) {
    for (u64 v = 0; v < g.node_cap(); ++v) {
        if (g.is_node_deleted(v)) continue;
        if (sel && !sel->has(v)) continue;
        nodes.push_back(v);
        values.push_back(value(v));
    }
}

// ---- algo.pageRank -------------------------------------------------------------------------------------
PageRankResult algo_pagerank(const Graph& g, const std::optional<std::string>& label,
                             const std::optional<std::string>& rel_type) {
    PageRankResult res;
    const u64 n = g.node_cap();
    const u64 live = g.live_nodes();
    if (live == 0) return res;                                           // node_count() == 0 (:699-701)
    std::vector<std::string> types;
    if (rel_type) types.push_back(*rel_type);
    // a label that covers every live node is the unfiltered run (:711-713); otherwise the labelled nodes form a
    // compact graph of their own (:725-733) — here the induced subgraph selected by a bitmap
    NodeSelection sel;
    bool filtered = false;
    if (label) {
        sel = select_nodes(g, {*label});
        if (sel.count == 0) return res;                                  // (no node carries an unknown label)
        filtered = sel.count != live;
    }
    Matrix adj = g.build_adjacency_matrix(types);                        // graph.rs:3870-3894
    std::vector<float> score(n);
    int32_t iters = 0;
    // deleted ids stay in the unfiltered matrix as isolated vertices (n = node_count + deleted_nodes_count, :718-720)
    Matrix adj_t = adj.transpose();                                      // LAGraph_Cached_AT (:736-737); cached per snapshot
    check(fgpu_pagerank(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), filtered ? sel.bits.data() : nullptr, 0.85f, 1e-4f, 100,
                        score.data(), &iters),
          "LAGr_PageRank");
    emit_rows(g, filtered ? &sel : nullptr, res.nodes, res.scores, [&](u64 v) { return (double)score[v]; });   // :768-770
    return res;
}

// ---- algo.WCC -------------------------------------------------------------------------------------------
WccResult algo_wcc(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types) {
    WccResult res;
    const u64 n = g.node_cap();
    if (g.live_nodes() == 0) return res;                                 // node_count() == 0 (:801-803)
    // labels: the union of the labels' live nodes as an induced subgraph — the reference's compact graph (:817-826)
    NodeSelection sel;
    const bool filtered = !labels.empty();
    if (filtered) {
        sel = select_nodes(g, labels);
        if (sel.count == 0) return res;                                  // :822-824
    }
    // the plain adjacency and its per-snapshot cached transpose: the undirected view without building A (+) A' per call
    // (build_symmetric_adjacency_matrix, :813); unknown types contribute no edges.  Deleted ids stay in the unfiltered run
    // as isolated vertices (n = node_count + deleted_nodes_count, :814-816).
    Matrix adj = g.build_adjacency_matrix(types);                        // graph.rs:3870-3894
    Matrix adj_t = adj.transpose();
    std::vector<int64_t> comp(n);
    check(fgpu_wcc(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), filtered ? sel.bits.data() : nullptr, comp.data(), nullptr),
          "LAGr_ConnectedComponents");
    // a filtered run's componentId is the representative's COMPACT index — its rank among the selected ids in ascending
    // order (:617-626) — which the reference never maps back to a node id (:854-868)
    const std::vector<int64_t> rank = filtered ? compact_ranks(sel, n) : std::vector<int64_t>();
    // (fgpu_wcc writes comp[v] = -1 exactly for the unselected v)
    emit_rows(g, filtered ? &sel : nullptr, res.nodes, res.component_ids,
              [&](u64 v) { return filtered ? rank[(size_t)comp[v]] : comp[v]; });   // :857-859
    return res;
}

// ---- algo.labelPropagation ------------------------------------------------------------------------------
CdlpResult algo_cdlp(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                     int64_t max_iterations) {
    if (max_iterations <= 0) throw std::invalid_argument("maxIterations must be a positive integer");   // :1184-1193
    CdlpResult res;
    const u64 n = g.node_cap();
    if (g.live_nodes() == 0) return res;                                 // node_count() == 0 (:1196-1198)
    // labels: the union of the labels' live nodes as an induced subgraph — the reference's compact graph (:1215-1222)
    NodeSelection sel;
    const bool filtered = !labels.empty();
    if (filtered) {
        sel = select_nodes(g, labels);
        if (sel.count == 0) return res;                                  // :1217-1219
    }
    // A (+) A' (:1208); unknown types contribute no edges.  Deleted ids stay in the unfiltered run as isolated vertices
    // (n = node_count + deleted_nodes_count, :1211-1212).
    Matrix sym = g.build_symmetric_adjacency_matrix(types);              // graph.rs:3898-3907
    std::vector<int64_t> comm(n);
    const int32_t itermax = max_iterations > INT32_MAX ? INT32_MAX : (int32_t)max_iterations;   // (`*n as i32`, :1190)
    check(fgpu_cdlp(g.ctx().raw(), sym.snapshot(), filtered ? sel.bits.data() : nullptr, itermax, comm.data(), nullptr),
          "LAGraph_cdlp");
    // a filtered run's communityId is the label's COMPACT index — its rank among the selected ids in ascending order — which
    // the reference never maps back to a node id (:1244-1258).  Exact: ranks keep the order of the ids, so every tie-break of
    // the compact run picks the same vertex
    const std::vector<int64_t> rank = filtered ? compact_ranks(sel, n) : std::vector<int64_t>();
    // (fgpu_cdlp writes comm[v] = -1 exactly for the unselected v)
    emit_rows(g, filtered ? &sel : nullptr, res.nodes, res.community_ids,
              [&](u64 v) { return filtered ? rank[(size_t)comm[v]] : comm[v]; });   // :1249-1258
    return res;
}

// ---- algo.HarmonicCentrality ----------------------------------------------------------------------------
// algo.HarmonicCentrality and algo.MSF refuse an unknown relationship type, the first one listed, before anything else
static void require_types(const Graph& g, const std::vector<std::string>& types) {
    for (auto& t : types)
        if (!g.type_id(t)) throw std::invalid_argument("Relationship type '" + t + "' does not exist");
}

HarmonicResult algo_harmonic_centrality(const Graph& g, const std::vector<std::string>& labels,
                                        const std::vector<std::string>& types) {
    require_types(g, types);                                             // before the empty-graph exit (:2648-2652)
    HarmonicResult res;
    const u64 n = g.node_cap();
    if (g.live_nodes() == 0) return res;                                 // node_count() == 0 (:2654-2656)
    // labels: the union of the labels' live nodes as an induced subgraph — the reference's compact graph (:2658-2666,
    // :2704-2708); the sketches hash the node ids, not the compact indices
    NodeSelection sel;
    const bool filtered = !labels.empty();
    if (filtered) {
        sel = select_nodes(g, labels);
        if (sel.count == 0) return res;                                  // :2664-2666
    }
    // the directed adjacency over the selected types (:2676).  Deleted ids stay in the unfiltered run as isolated vertices
    // (n = node_count + deleted_nodes_count, :2701-2702) and leave the rows (:2760-2762).
    Matrix adj = g.build_adjacency_matrix(types);                        // graph.rs:3870-3894
    std::vector<double> score(n);
    std::vector<int64_t> reach(n);
    check(fgpu_harmonic(g.ctx().raw(), adj.snapshot(), filtered ? sel.bits.data() : nullptr, score.data(), reach.data(), nullptr,
                        nullptr),
          "LAGr_HarmonicCentrality");
    for (u64 v = 0; v < n; ++v) {                                        // :2755-2767
        if (g.is_node_deleted(v)) continue;
        if (filtered && !sel.has(v)) continue;
        res.nodes.push_back(v);
        res.scores.push_back(score[v]);
        res.reachable.push_back(reach[v]);
    }
    return res;
}

// ---- the algorithms' weighted pair matrix (fgpu_pair_weights) ---------------------------------------------
namespace {
// An attribute list (edge_ids[k], vals[k]) in any order as fgpu_pair_weights takes it: the ids strictly ascending.  Of equal ids
// the last one stands, which is what assigning them to a map in turn gave.  A list that ascends already is passed through.
struct AttrList {
    const u64* ids = nullptr;   // nullptr: no such attribute, every relationship weighs 1.0
    const double* vals = nullptr;
    u64 n = 0;
    std::vector<u64> own_ids;
    std::vector<double> own_vals;
    AttrList(const u64* edge_ids, const double* v, u64 count) {
        static const u64 no_id = 0;
        static const double no_val = 0.0;
        if (!edge_ids) return;
        ids = &no_id; vals = &no_val;                                    // (a list of nothing is still a list)
        if (count == 0) return;
        bool ascending = true;
        for (u64 k = 1; k < count && ascending; ++k) ascending = edge_ids[k - 1] < edge_ids[k];
        if (ascending) { ids = edge_ids; vals = v; n = count; return; }
        std::vector<u64> order(count);
        for (u64 k = 0; k < count; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) { return edge_ids[a] < edge_ids[b]; });
        own_ids.reserve(count); own_vals.reserve(count);
        for (u64 k = 0; k < count; ++k) {
            if (k + 1 < count && edge_ids[order[k + 1]] == edge_ids[order[k]]) continue;   // a later one of the same id follows
            own_ids.push_back(edge_ids[order[k]]);
            own_vals.push_back(v[order[k]]);
        }
        ids = own_ids.data(); vals = own_vals.data(); n = own_ids.size();
    }
};

// W (weights, or the BOOL pattern without an attribute) and K (the kept relationship per pair) over the tensors' own layers
struct PairMatrices {
    SnapshotRef w, k;
    std::optional<Matrix> none;   // no tensor is selected: one empty n x n matrix stands for both
    const fgpu_mat* W() const { return none ? none->snapshot() : w.get(); }
    const fgpu_mat* K() const { return none ? none->snapshot() : k.get(); }
};
PairMatrices device_pair_weights(const Graph& g, const std::vector<u64>& tids, int flags, const u64* active, const AttrList& attr,
                                 double missing, const char* who, bool want_k = true) {
    PairMatrices out;
    u64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (tids.empty()) {
        out.none.emplace(g.ctx(), attr.ids ? Type::UInt64 : Type::Bool, g.node_cap(), g.node_cap());
        g.set_pair_stats(stats);
        return out;
    }
    std::vector<const fgpu_mat*> m, dp, dm;
    std::vector<const fgpu_multi*> multi;
    for (u64 t : tids) {
        const Tensor& ten = g.relationship_tensors()[t];
        ten.wait_fwd();
        const Layers f = fwd_layers(ten);
        m.push_back(f.m); dp.push_back(f.dp); dm.push_back(f.dm);
        multi.push_back(ten.multi_table());
    }
    u64 refused = ~0ull;
    const fgpu_info info = fgpu_pair_weights(g.ctx().raw(), m.data(), dp.data(), dm.data(), multi.data(), (int)tids.size(), flags, active,
                                             attr.ids, attr.vals, attr.n, missing, out.w.out(), want_k ? out.k.out() : nullptr, &refused, stats);
    g.set_pair_stats(stats);
    if (info == FGPU_INVALID && refused != ~0ull)
        throw std::invalid_argument(std::string(who) + ": relationship " + std::to_string(refused) + " has a negative weight");
    check(info, who);
    return out;
}

// the kept relationship of every (rows[i], cols[i]), i < n: one batched probe of K
std::vector<u64> kept_relationships(const Graph& g, const fgpu_mat* K, const u64* rows, const u64* cols, u64 n, const char* who) {
    std::vector<u64> kept(n);
    if (n == 0) return kept;
    std::vector<uint8_t> present(n);
    check(fgpu_mat_probe(g.ctx().raw(), K, rows, cols, n, present.data(), kept.data()), who);
    for (u64 i = 0; i < n; ++i)
        if (!present[i]) throw std::runtime_error(std::string(who) + ": a chosen pair has no kept relationship");
    return kept;
}
}  // namespace

// ---- algo.MSF -------------------------------------------------------------------------------------------
MsfResult algo_msf(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types, bool maximize,
                   const u64* edge_ids, const double* weights, u64 n_weights) {
    require_types(g, types);                                             // before the empty-graph exit (:1287-1295)
    MsfResult res;
    const u64 n = g.node_cap();
    if (g.live_nodes() == 0) return res;                                 // node_count() == 0 (:1323-1325)
    // the nodes of the run: the labels' live nodes, or every live node (collect_node_ids, :1328-1331).  The reference
    // renumbers them 0..k-1; here they are an induced subgraph, and the order of the ids — all the forest depends on — is kept
    const NodeSelection sel = labels.empty() ? select_live_nodes(g) : select_nodes(g, labels);
    if (sel.count == 0) return res;
    const std::vector<u64> tids = scanned_type_ids(g, types);
    // One (score, relationship) per unordered pair, on the device: the score of a relationship is msf_score (:143-165) — 1.0
    // without a weight attribute, +inf when it has none (under either objective), negated under maximize — over the selected
    // tensors' effective edges, multi-edges included, both directions folded together, ties to the smallest id
    // (msf_keep_min_score, :237-255).  W is the symmetric weighted matrix of weighted_adj (:1690-1704), BOOL in the unit case.
    const AttrList attr(edge_ids, weights, n_weights);
    const PairMatrices pm = device_pair_weights(g, tids, FGPU_PAIRS_OUT | FGPU_PAIRS_IN | (maximize ? FGPU_PAIRS_NEGATE : 0),
                                                sel.bits.data(), attr, std::numeric_limits<double>::infinity(), "algo.MSF");
    std::vector<int64_t> comp(n);
    EdgeList forest(g.ctx());
    msf(g.ctx(), pm.W(), sel.bits.data(), comp.data(), forest);
    // trees in ascending order of their smallest node id = their component label (:1778-1848)
    std::vector<int64_t> tree_of(n, -1);
    for (u64 v = 0; v < n; ++v) {
        if (comp[v] < 0) continue;
        if ((u64)comp[v] == v) {
            tree_of[v] = (int64_t)res.tree_nodes.size();
            res.tree_nodes.emplace_back();
            res.tree_edges.emplace_back();
        }
        res.tree_nodes[(size_t)tree_of[(size_t)comp[v]]].push_back(v);   // (comp[v] <= v: its tree exists already)
    }
    const std::vector<u64> kept = kept_relationships(g, pm.K(), forest.rows.p, forest.cols.p, forest.n, "algo.MSF");
    for (u64 i = 0; i < forest.n; ++i) res.tree_edges[(size_t)tree_of[(size_t)comp[forest.rows[i]]]].push_back(kept[i]);
    return res;
}

// ---- algo.maxFlow ---------------------------------------------------------------------------------------
MaxFlowResult algo_maxflow(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                           const std::vector<u64>& sources, const std::vector<u64>& targets, bool has_attribute,
                           const u64* edge_ids, const double* caps, u64 n_caps, bool has_default, double default_capacity) {
    if (types.size() != 1)                                               // :2809-2813
        throw std::invalid_argument("algo.maxFlow: exactly one relationship type must be given in 'relationshipTypes'");
    if (sources.empty() || targets.empty())                              // :2841-2845
        throw std::invalid_argument("algo.maxFlow expects at least one source node and one target node");
    const std::unordered_set<u64> src_set(sources.begin(), sources.end());
    for (u64 t : targets)                                                // :2847-2853
        if (src_set.count(t)) throw std::invalid_argument("algo.maxFlow: the source set and the target set must be disjoint");
    if (has_default && !(default_capacity >= 0.0))                       // :2864-2875
        throw std::invalid_argument("algo.maxFlow: 'defaultCapacity' must be a number that is not negative");
    const auto tid = g.type_id(types[0]);
    if (!tid) throw std::invalid_argument("algo.maxFlow: relationship type '" + types[0] + "' is unknown");   // :2879-2884
    const Tensor& tensor = g.relationship_tensors()[*tid];
    if (tensor.has_multi_edge())                                         // :2885-2890
        throw std::invalid_argument("algo.maxFlow: relationship type '" + types[0] +
                                    "' holds multi-edges, which a capacity matrix cannot express");
    const char* no_capacity = "algo.maxFlow: a relationship has an invalid or missing attribute and no default capacity was given";
    if (!has_attribute && !has_default) throw std::invalid_argument(no_capacity);   // :2894-2898
    NodeSelection sel;
    const bool filtered = !labels.empty();
    if (filtered) sel = select_nodes(g, labels);                         // :2900-2905
    std::unordered_map<u64, double> attr;
    if (has_attribute && edge_ids) {
        attr.reserve(n_caps * 2);
        for (u64 k = 0; k < n_caps; ++k) attr[edge_ids[k]] = caps[k];
    }
    // the type's effective edges whose two ends are selected, each with its capacity (:2907-2951)
    struct Arc { u64 src, dst, edge; double cap; };
    std::vector<Arc> arcs;
    for (const Entry& e : tensor.iter_edges()) {
        if (filtered && (!sel.has(e.row) || !sel.has(e.col))) continue;
        double c = default_capacity;
        const auto it = attr.find(e.val);
        if (it != attr.end() && it->second >= 0.0) c = it->second;
        else if (!has_default) throw std::invalid_argument(no_capacity);
        arcs.push_back(Arc{e.row, e.col, e.val, c});
    }
    MaxFlowResult res;
    if (arcs.empty()) return res;                                        // one row of three empty lists and 0.0 (:2953-2960)
    const bool multi_src = sources.size() > 1, multi_sink = targets.size() > 1;
    // identity ids when nothing was filtered out and no id is a tombstone, else the sorted distinct ends (:2965-3102)
    const bool identity = !filtered && g.deleted_nodes_count() == 0;
    std::vector<u64> compact_to_id;
    std::unordered_map<u64, u64> id_to_compact;
    u64 base = g.node_cap();
    if (!identity) {
        compact_to_id.assign(sources.begin(), sources.end());
        compact_to_id.insert(compact_to_id.end(), targets.begin(), targets.end());
        for (const Arc& a : arcs) { compact_to_id.push_back(a.src); compact_to_id.push_back(a.dst); }
        std::sort(compact_to_id.begin(), compact_to_id.end());
        compact_to_id.erase(std::unique(compact_to_id.begin(), compact_to_id.end()), compact_to_id.end());
        for (u64 k = 0; k < compact_to_id.size(); ++k) id_to_compact[compact_to_id[k]] = k;
        base = compact_to_id.size();
    }
    auto compact = [&](u64 id) { return identity ? id : id_to_compact.at(id); };
    for (u64 v : sources)
        if (identity && v >= base) throw std::invalid_argument("algo.maxFlow: a source node is not in the graph");
    for (u64 v : targets)
        if (identity && v >= base) throw std::invalid_argument("algo.maxFlow: a target node is not in the graph");
    const u64 super_src = base, super_sink = base + (multi_src ? 1 : 0);
    const u64 total = base + (multi_src ? 1 : 0) + (multi_sink ? 1 : 0);
    std::vector<u64> rows, cols, bits;
    std::vector<const Arc*> kept;                                        // the arcs with capacity > 0, in tensor order
    double min_cap = std::numeric_limits<double>::infinity(), max_cap = 0.0;
    auto add = [&](u64 u, u64 v, double c) {
        u64 b;
        memcpy(&b, &c, sizeof b);
        rows.push_back(u); cols.push_back(v); bits.push_back(b);
    };
    for (const Arc& a : arcs) {
        if (!(a.cap > 0.0)) continue;
        add(compact(a.src), compact(a.dst), a.cap);
        kept.push_back(&a);
        if (a.cap < min_cap) min_cap = a.cap;
        if (a.cap > max_cap) max_cap = a.cap;
    }
    const double big = 2147483647.0;                                     // i32::MAX
    u64 src_id = compact(sources[0]), sink_id = compact(targets[0]);
    if (multi_src) {
        src_id = super_src;
        std::unordered_set<u64> once;                                    // (a node listed twice hangs under it once)
        for (u64 v : sources)
            if (once.insert(v).second) add(src_id, compact(v), big);
    }
    if (multi_sink) {
        sink_id = super_sink;
        std::unordered_set<u64> once;
        for (u64 v : targets)
            if (once.insert(v).second) add(compact(v), sink_id, big);
    }
    if (std::isfinite(min_cap) && max_cap >= min_cap * 4294967295.0)     // :3104-3110
        throw std::invalid_argument("algo.maxFlow: capacity range too wide: the largest capacity is at least 2^32 - 1 times the "
                                    "smallest, which the solver's arithmetic cannot keep apart");
    Matrix cap(g.ctx(), Type::UInt64, total, total);
    if (!rows.empty()) cap.build(rows, cols, &bits);                     // (every position once: no multi-edge, super arcs once)
    EdgeList flow(g.ctx());
    maxflow(g.ctx(), cap.snapshot(), src_id, sink_id, &res.max_flow, flow);
    std::unordered_map<u64, double> flow_of;                             // (row << 32 | col) -> flow; ids fit 32 bits (fgpu_maxflow)
    flow_of.reserve(flow.n * 2);
    for (u64 i = 0; i < flow.n; ++i) flow_of[(flow.rows[i] << 32) | flow.cols[i]] = flow.vals[i];
    std::set<u64> used;
    for (const Arc* a : kept) {                                          // :3218-3232
        const auto it = flow_of.find((compact(a->src) << 32) | compact(a->dst));
        if (it == flow_of.end() || it->second == 0.0) continue;
        used.insert(a->src);
        used.insert(a->dst);
        res.edges.push_back(a->edge);
        res.flows.push_back(it->second);
    }
    res.nodes.assign(used.begin(), used.end());
    return res;
}

// ---- algo.SPpaths / algo.SSpaths ------------------------------------------------------------------------
namespace {
// the tensors a relTypes list selects are scanned_type_ids; the enumeration keeps a repeated name — its successors come twice —
// and the weight matrices, one entry per pair either way, take each tensor once
std::vector<u64> each_once(const std::vector<u64>& tids) {
    std::vector<u64> out;
    for (u64 t : tids)
        if (std::find(out.begin(), out.end(), t) == out.end()) out.push_back(t);
    return out;
}

// weightProp / costProp as data: edge_numeric_attr (:2049-2062)
struct PathAttrs {
    bool unit = true;
    std::unordered_map<u64, double> wattr, cattr;
    PathAttrs(const u64* w_edge_ids, const double* w_vals, u64 n_w, const u64* c_edge_ids, const double* c_vals, u64 n_c)
        : unit(w_edge_ids == nullptr) {
        if (!unit) {
            wattr.reserve(n_w * 2);
            for (u64 k = 0; k < n_w; ++k) wattr[w_edge_ids[k]] = w_vals[k];
        }
        if (c_edge_ids) {
            cattr.reserve(n_c * 2);
            for (u64 k = 0; k < n_c; ++k) cattr[c_edge_ids[k]] = c_vals[k];
        }
    }
    double weight(u64 edge) const {
        if (unit) return 1.0;
        const auto it = wattr.find(edge);
        return it != wattr.end() ? it->second : 1.0;
    }
    double cost(u64 edge) const {
        const auto it = cattr.find(edge);
        return it != cattr.end() ? it->second : 0.0;
    }
};

// The weight matrix of a search in traversal direction `dir`, on the device: one (weight, relationship) per ordered pair
// (from, to), the smallest weight over the selected tensors and their multi-edges, ties to the smallest id; self-loops and
// non-finite weights (never relaxed, :2213) left out, an unlisted relationship weighs 1.0, a negative weight throws
PairMatrices path_pair_weights(const Graph& g, const std::vector<u64>& tids, Direction dir, const AttrList& weight, bool want_k = true,
                               const char* who = "algo.SPpaths") {
    const int flags = (dir != Direction::Incoming ? FGPU_PAIRS_OUT : 0) | (dir != Direction::Outgoing ? FGPU_PAIRS_IN : 0) |
                      FGPU_PAIRS_DROP_NONFINITE | FGPU_PAIRS_REFUSE_NEGATIVE;
    return device_pair_weights(g, tids, flags, nullptr, weight, 1.0, who, want_k);
}

// path_pair_weights' refusal alone, for the walks that need no matrix: the same relationships, the same message
void refuse_negative_weights(const Graph& g, const std::vector<u64>& tids, const PathAttrs& at, const char* who) {
    if (at.unit) return;
    for (u64 t : tids)
        for (const Entry& e : g.relationship_tensors()[t].iter_edges()) {
            if (e.row == e.col) continue;
            const double w = at.weight(e.val);
            if (std::isfinite(w) && w < 0.0)
                throw std::invalid_argument(std::string(who) + ": relationship " + std::to_string(e.val) + " has a negative weight");
        }
}

}  // namespace

SpPathResult algo_sp_paths(const Graph& g, u64 source, u64 target, const std::vector<std::string>& types, Direction dir,
                           const u64* w_edge_ids, const double* w_vals, u64 n_w,
                           const u64* c_edge_ids, const double* c_vals, u64 n_c) {
    SpPathResult res;
    const u64 n = g.node_cap();
    if (source == target) return res;                                    // :2559-2567
    if (source >= n || target >= n || g.is_node_deleted(source) || g.is_node_deleted(target)) return res;
    const PathAttrs at(nullptr, nullptr, 0, c_edge_ids, c_vals, n_c);   // (the costs alone: the weights stay a list for the device)
    const PairMatrices pm = path_pair_weights(g, each_once(scanned_type_ids(g, types)), dir, AttrList(w_edge_ids, w_vals, n_w));
    std::vector<double> dist(n);
    std::vector<int64_t> parent(n);
    sssp(g.ctx(), pm.W(), source, dist.data(), parent.data());
    if (!std::isfinite(dist[target])) return res;
    res.found = true;
    res.weight = dist[target];
    for (u64 v = target, steps = 0; v != source; v = (u64)parent[v]) {
        if (++steps > n || parent[v] < 0 || (u64)parent[v] >= n)
            throw std::runtime_error("algo.SPpaths: the parent chain does not lead back to the source");
        res.nodes.push_back(v);
    }
    res.nodes.push_back(source);
    std::reverse(res.nodes.begin(), res.nodes.end());
    res.edges = kept_relationships(g, pm.K(), res.nodes.data(), res.nodes.data() + 1, res.nodes.size() - 1, "algo.SPpaths");
    for (u64 edge : res.edges) res.cost += at.cost(edge);               // :2250-2254
    return res;
}

namespace {
// cmp_found_path (:2037-2045): ascending weight, then cost, then hop count (the values are finite: partial_cmp never fails)
int cmp_path(const PathRow& a, const PathRow& b) {
    if (a.weight != b.weight) return a.weight < b.weight ? -1 : 1;
    if (a.cost != b.cost) return a.cost < b.cost ? -1 : 1;
    if (a.edges.size() != b.edges.size()) return a.edges.size() < b.edges.size() ? -1 : 1;
    return 0;
}

// record_found_path (:2350-2403)
void record_path(std::vector<PathRow>& results, PathRow&& found, int64_t path_count, double& bound) {
    if (path_count == 1) {
        if (results.empty() || cmp_path(found, results.front()) < 0) {
            bound = found.weight;
            results.clear();
            results.push_back(std::move(found));
        }
        return;
    }
    if (path_count == 0) {
        if (results.empty()) {
            bound = found.weight;
            results.push_back(std::move(found));
        } else if (found.weight > results.front().weight) {
        } else if (found.weight < results.front().weight) {
            bound = found.weight;
            results.clear();
            results.push_back(std::move(found));
        } else {
            results.push_back(std::move(found));
        }
        return;
    }
    const size_t k = (size_t)path_count;
    if (results.size() == k) {
        if (cmp_path(found, results[k - 1]) >= 0) return;
        results.pop_back();
    }
    const auto pos = std::partition_point(results.begin(), results.end(), [&](const PathRow& kept) { return cmp_path(kept, found) < 0; });
    results.insert(pos, std::move(found));
    if (results.size() == k) bound = results[k - 1].weight;
}

// what prunes the walk: `rows` rows of n lower bounds on the weight left to the target (rows == 1: one row for every budget)
struct PathTable {
    std::vector<double> d;
    u64 n = 0;
    uint32_t rows = 0;
    double slack = 0.0;
    double at(uint32_t left, u64 v) const { return d[(size_t)(rows == 1 ? 0 : left) * n + v]; }
};

// enumerate_paths (:2414-2514) + the final sort (:2595); `table` nullable
std::vector<PathRow> enumerate_paths(const Graph& g, u64 source, std::optional<u64> target, const PathQuery& q, const PathAttrs& at,
                                     const PathTable* table, double bound, PathEnumStats& st) {
    struct Succ { u64 edge, far; };
    struct Live { u64 edge; double weight, cost; };                      // the PREFIX sums up to and including this edge
    const std::vector<u64> tids = scanned_type_ids(g, q.types);
    const bool with_out = q.dir != Direction::Incoming, with_in = q.dir != Direction::Outgoing;
    auto successors = [&](u64 node) {                                    // node_successors (:2098-2109)
        std::vector<Succ> out;
        for (const VlEdge& e : node_relationships(g, node, tids, with_out, with_in))
            out.push_back({e.id, with_out && e.src == node ? e.dst : e.src});   // far_endpoint (:2066-2085)
        return out;
    };
    std::vector<std::optional<std::vector<Succ>>> levels;
    std::vector<u64> nodes{source};
    std::vector<Live> live;
    std::vector<uint8_t> on_path(g.node_cap(), 0);
    on_path[source] = 1;
    levels.push_back(q.max_len > 0 ? std::optional<std::vector<Succ>>(successors(source)) : std::nullopt);
    std::vector<PathRow> results;
    for (;;) {
        const size_t depth = live.size();
        auto& lv = levels[depth];
        if (lv && !lv->empty()) {
            const Succ s = lv->back();
            lv->pop_back();
            ++st.examined;
            if (q.max_examined && st.examined > q.max_examined)
                throw std::runtime_error("algo.SPpaths: the enumeration spent its budget of " + std::to_string(q.max_examined) +
                                         " examined successors");
            if (on_path[s.far]) continue;                                // simple paths only
            const double w0 = live.empty() ? 0.0 : live.back().weight, c0 = live.empty() ? 0.0 : live.back().cost;
            const double next_weight = w0 + at.weight(s.edge), next_cost = c0 + at.cost(s.edge);
            if (!std::isfinite(next_weight) || next_weight > bound) continue;
            if (!std::isfinite(next_cost) || (q.max_cost && next_cost > *q.max_cost)) continue;
            if (table) {
                const double left = table->at(q.max_len - (uint32_t)(depth + 1), s.far);
                if (std::isinf(left)) { ++st.pruned_hops; continue; }
                if ((next_weight + left) * (1.0 - table->slack) > bound) { ++st.pruned_weight; continue; }
            }
            live.push_back({s.edge, next_weight, next_cost});
            nodes.push_back(s.far);
            on_path[s.far] = 1;
            const bool at_target = !target || s.far == *target;
            if (at_target) {
                PathRow found;
                found.nodes = nodes;
                for (const Live& e : live) found.edges.push_back(e.edge);
                found.weight = next_weight;
                found.cost = next_cost;
                record_path(results, std::move(found), q.path_count, bound);
            }
            const bool expand = !(at_target && target) && live.size() < (size_t)q.max_len;
            levels.push_back(expand ? std::optional<std::vector<Succ>>(successors(s.far)) : std::nullopt);
        } else {
            if (depth == 0) break;
            levels.pop_back();
            live.pop_back();
            on_path[nodes.back()] = 0;
            nodes.pop_back();
        }
    }
    std::stable_sort(results.begin(), results.end(), [](const PathRow& a, const PathRow& b) { return cmp_path(a, b) < 0; });
    return results;
}

// bfs_find_bound's answer (:2267-2320) without its weight: is there a route source -> target of at most maxLen arcs?
bool reachable_within(const Graph& g, u64 source, u64 target, const PathQuery& q) {
    const std::vector<u64> tids = scanned_type_ids(g, q.types);
    const bool with_out = q.dir != Direction::Incoming, with_in = q.dir != Direction::Outgoing;
    std::vector<uint8_t> seen(g.node_cap(), 0);
    std::vector<u64> frontier{source}, next;
    seen[source] = 1;
    for (u64 hop = 0; hop < q.max_len && !frontier.empty(); ++hop) {
        next.clear();
        for (u64 u : frontier)
            for (const VlEdge& e : node_relationships(g, u, tids, with_out, with_in)) {
                const u64 far = with_out && e.src == u ? e.dst : e.src;
                if (seen[far]) continue;
                if (far == target) return true;
                seen[far] = 1;
                next.push_back(far);
            }
        frontier.swap(next);
    }
    return false;
}

void check_path_count(const PathQuery& q) {
    if (q.path_count < 0) throw std::invalid_argument("pathCount must be a non-negative integer");   // :1940
}
}  // namespace

std::vector<PathRow> algo_sp_paths_rows(const Graph& g, u64 source, u64 target, const PathQuery& q, PathEnumStats* stats) {
    PathEnumStats local;
    PathEnumStats& st = stats ? *stats : local;
    st = PathEnumStats();
    check_path_count(q);
    if (q.path_count == 1 && !q.max_cost && q.max_len == UINT32_MAX && source != target) {   // the fast shape (:2563-2571)
        st.table_rows = 0;
        SpPathResult one = algo_sp_paths(g, source, target, q.types, q.dir, q.w_edge_ids, q.w_vals, q.n_w, q.c_edge_ids, q.c_vals, q.n_c);
        std::vector<PathRow> rows;
        if (one.found) rows.push_back({std::move(one.nodes), std::move(one.edges), one.weight, one.cost});
        return rows;
    }
    const u64 n = g.node_cap();
    const PathAttrs at(q.w_edge_ids, q.w_vals, q.n_w, q.c_edge_ids, q.c_vals, q.n_c);
    const std::vector<u64> once = each_once(scanned_type_ids(g, q.types));
    refuse_negative_weights(g, once, at, "algo.SPpaths");                // (pruning or not, whatever the nodes are)
    if (source >= n || target >= n || g.is_node_deleted(source) || g.is_node_deleted(target)) return {};
    if (source == target) return {};         // bfs_find_bound never "finds" the source it starts from: None (:2278-2279)
    const double inf = std::numeric_limits<double>::infinity();
    if (!q.prune) {
        // bfs_find_bound's None: no route within maxLen, no enumeration — without it an unreachable target costs every simple
        // path of the component.  Its weight is not used as a seed: the rows do not depend on the seed.
        if (!reachable_within(g, source, target, q)) return {};
        return enumerate_paths(g, source, target, q, at, nullptr, inf, st);
    }
    const Direction rev = q.dir == Direction::Outgoing ? Direction::Incoming : q.dir == Direction::Incoming ? Direction::Outgoing : Direction::Both;
    const PairMatrices wrev = path_pair_weights(g, once, rev, AttrList(q.w_edge_ids, q.w_vals, q.n_w), false);   // (the table needs no K)
    PathTable table;
    table.n = n;
    const bool hop_table = q.max_len <= (uint32_t)FGPU_SSSP_HOPS_MAX && ((u64)q.max_len + 1) * n * sizeof(double) <= (1ull << 30);
    if (hop_table) {
        table.rows = q.max_len + 1;
        table.d.resize((size_t)table.rows * n);
        sssp_hops(g.ctx(), wrev.W(), target, (int32_t)q.max_len, table.d.data());
        st.table_rows = (int32_t)table.rows;
    } else {
        table.rows = 1;
        table.d.resize(n);
        sssp(g.ctx(), wrev.W(), target, table.d.data(), nullptr);
        st.table_rows = 0;
    }
    const u64 m = std::min<u64>(q.max_len, n - 1) + 1;
    table.slack = 8.0 * (double)m * std::ldexp(1.0, -53);
    const double reach = table.at(q.max_len, source);
    if (std::isinf(reach)) return {};                                    // bfs_find_bound's None (:2579-2581)
    // The one row of the fallback knows no hop budget.  It bounds every completion from below, so it may prune; but it is the
    // weight of a QUALIFYING path only when a simple path cannot be longer than maxLen anyway (maxLen >= n - 1, "no maxLen"
    // included).  Below that the cheapest route may need more than maxLen arcs: the row then neither seeds the bound (every
    // qualifying path would lie above it) nor answers bfs_find_bound's question, which the host BFS answers instead.
    const bool exact = hop_table || (u64)q.max_len >= n - 1;
    if (!exact && !reachable_within(g, source, target, q)) return {};
    const double seed = (exact && q.path_count <= 1 && !q.max_cost) ? reach * (1.0 + table.slack) : inf;
    return enumerate_paths(g, source, target, q, at, &table, seed, st);
}

std::vector<PathRow> algo_ss_paths(const Graph& g, u64 source, const PathQuery& q, PathEnumStats* stats) {
    PathEnumStats local;
    PathEnumStats& st = stats ? *stats : local;
    st = PathEnumStats();
    check_path_count(q);
    const PathAttrs at(q.w_edge_ids, q.w_vals, q.n_w, q.c_edge_ids, q.c_vals, q.n_c);
    refuse_negative_weights(g, each_once(scanned_type_ids(g, q.types)), at, "algo.SSpaths");
    if (source >= g.node_cap() || g.is_node_deleted(source)) return {};
    return enumerate_paths(g, source, std::nullopt, q, at, nullptr, std::numeric_limits<double>::infinity(), st);
}

// ---- algo.betweenness -----------------------------------------------------------------------------------
std::vector<u64> betweenness_sources(u64 n_nodes, int64_t sampling_size, int64_t sampling_seed) {
    if (sampling_size <= 0) throw std::invalid_argument("samplingSize must be a positive integer");   // :900-905
    // `*n as i32` keeps the low 32 bits, `as usize` sign-extends them: 2^32 + 5 -> 5, 2^31 -> 2^64 - 2^31 ("all nodes")
    const u64 size = (u64)(int64_t)(int32_t)(uint32_t)(uint64_t)sampling_size;
    const u64 seed = (u64)sampling_seed;                                 // `*n as u64`: negative seeds wrap (:909-913)
    std::vector<u64> out;
    if (n_nodes == 0) return out;                                        // :954-955
    if (size >= n_nodes) {                                               // :956-957
        out.resize(n_nodes);
        for (u64 i = 0; i < n_nodes; ++i) out[i] = i;
        return out;
    }
    std::vector<uint8_t> used(n_nodes, 0);
    u64 rng = seed;
    for (u64 i = 0; i < size; ++i) {                                     // :958-974
        u64 idx;
        if (seed == 0) {
            idx = i % n_nodes;
        } else {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            idx = (rng >> 33) % n_nodes;
        }
        if (!used[idx]) {
            used[idx] = 1;
            out.push_back(idx);
        }
    }
    return out;
}

BetweennessResult algo_betweenness(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                                   int64_t sampling_size, int64_t sampling_seed) {
    BetweennessResult res;
    const u64 n = g.node_cap();
    if (sampling_size <= 0) throw std::invalid_argument("samplingSize must be a positive integer");   // before the graph (:900-905)
    if (g.live_nodes() == 0) return res;                                 // node_count() == 0 (:916-918)
    // labels: the union of the labels' live nodes as an induced subgraph — the reference's compact graph (:935-940)
    NodeSelection sel;
    std::vector<u64> selected;                                           // compact index -> node id (compact_to_id)
    const bool filtered = !labels.empty();
    if (filtered) {
        sel = select_nodes(g, labels, &selected);
        if (selected.empty()) return res;
    }
    // n_nodes: node_count + deleted_nodes_count unfiltered (deleted ids stay as vertices and can be sources), else the
    // selected nodes (:949-952)
    std::vector<u64> sources = betweenness_sources(filtered ? selected.size() : n, sampling_size, sampling_seed);
    if (filtered)
        for (auto& s : sources) s = selected[s];
    Matrix adj = g.build_adjacency_matrix(types);                        // graph.rs:3870-3894; unknown types add no edges
    Matrix adj_t = adj.transpose();                                      // LAGraph_Cached_AT (:945)
    std::vector<double> cent(n);
    check(fgpu_betweenness(g.ctx().raw(), adj.snapshot(), adj_t.snapshot(), filtered ? sel.bits.data() : nullptr, sources.data(),
                           sources.size(), cent.data(), nullptr),
          "LAGr_Betweenness");
    emit_rows(g, filtered ? &sel : nullptr, res.nodes, res.scores, [&](u64 v) { return cent[v]; });   // :1003-1005
    return res;
}

}  // namespace falkor
