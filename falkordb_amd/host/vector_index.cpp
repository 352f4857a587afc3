// vector_index.cpp — the vector indexes of a Graph and the two procedures that read them: db.idx.vector.queryNodes
// (runtime/ops/node_by_vector_scan.rs -> Graph::vector_query_nodes, graph.rs:3408-3457) and db.idx.vector.queryRelationships
// (edge_by_vector_scan.rs -> Graph::vector_query_edges).  The reference keeps an HNSW graph per index inside RediSearch
// (index/mod.rs:1768-1823), takes its k candidates, recomputes their distances and sorts them; here an index is an fgpu_vecidx
// and a whole parent batch is one exhaustive fgpu_vecidx_knn call, whose rows already come in ascending (distance, id).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "host.hpp"

namespace falkor {

int vector_metric(const char* similarity) {
    if (!similarity || !strcmp(similarity, "euclidean")) return FGPU_VEC_EUCLIDEAN;
    if (!strcmp(similarity, "cosine")) return FGPU_VEC_COSINE;
    if (!strcmp(similarity, "ip")) return FGPU_VEC_IP;
    throw std::runtime_error(std::string("Unknown similarity function '") + similarity + "', expected 'euclidean', 'ip', or 'cosine'");
}

static std::string dim_mismatch(u64 expected, u64 got) {
    return "Vector dimension mismatch, expected " + std::to_string(expected) + " but got " + std::to_string(got);
}

double vec_distance(int metric, const float* a, u64 na, const float* b, u64 nb) {
    if (na != nb) throw std::runtime_error(dim_mismatch(na, nb));
    double acc = 0.0, aa = 0.0, bb = 0.0;
    for (u64 i = 0; i < na; ++i) {
        const double x = (double)a[i], y = (double)b[i];
        if (metric == FGPU_VEC_EUCLIDEAN) acc += (x - y) * (x - y);
        else { acc += x * y; aa += x * x; bb += y * y; }
    }
    if (metric == FGPU_VEC_EUCLIDEAN) return sqrt(acc);
    if (metric == FGPU_VEC_IP) return -acc;
    return (aa == 0.0 || bb == 0.0) ? 1.0 : 1.0 - acc / (sqrt(aa) * sqrt(bb));
}

const VectorIndex* Graph::vector_index(bool is_edge, u64 owner, const std::string& attr) const {
    auto it = vec_indexes_.find(std::make_tuple(is_edge, owner, attr));
    return it == vec_indexes_.end() ? nullptr : it->second.get();
}

void Graph::vector_index_create(bool is_edge, u64 owner, const std::string& attr, u64 dim, const char* similarity) {
    const int metric = vector_metric(similarity);
    if (vector_index(is_edge, owner, attr)) throw std::runtime_error("Attribute '" + attr + "' is already indexed");
    if (dim < 1 || dim > FGPU_VECIDX_DIM_MAX)
        throw std::runtime_error("Vector index dimension must be 1 .. " + std::to_string(FGPU_VECIDX_DIM_MAX));
    auto vi = std::make_unique<VectorIndex>();
    vi->ctx = ctx_->raw();
    vi->dim = (uint32_t)dim;
    vi->metric = metric;
    check(fgpu_vecidx_new(vi->ctx, &vi->idx, vi->dim, metric), "db.idx.vector.create");
    vec_indexes_[std::make_tuple(is_edge, owner, attr)] = std::move(vi);
}

bool Graph::vector_index_drop(bool is_edge, u64 owner, const std::string& attr) {
    return vec_indexes_.erase(std::make_tuple(is_edge, owner, attr)) != 0;
}

static VectorIndex& index_or_throw(const VectorIndex* vi, const std::string& attr, u64 n) {
    if (!vi) throw std::runtime_error("No vector index on attribute '" + attr + "'");
    if (n != vi->dim) throw std::runtime_error(dim_mismatch(vi->dim, n));
    return *const_cast<VectorIndex*>(vi);
}

void Graph::vector_set_node(LabelId label, const std::string& attr, u64 node, const float* vec, u64 n) {
    VectorIndex& vi = index_or_throw(vector_index(false, label, attr), attr, n);
    check(fgpu_vecidx_set(vi.ctx, vi.idx, &node, vec, 1), "db.idx.vector.set");
}

void Graph::vector_set_edge(u64 type, const std::string& attr, u64 src, u64 dst, u64 edge_id, const float* vec, u64 n) {
    VectorIndex& vi = index_or_throw(vector_index(true, type, attr), attr, n);
    check(fgpu_vecidx_set(vi.ctx, vi.idx, &edge_id, vec, 1), "db.idx.vector.set");
    vi.ends[edge_id] = {src, dst};
}

static bool unset(VectorIndex* vi, u64 entity) {
    if (!vi) return false;
    uint64_t removed = 0;
    check(fgpu_vecidx_remove(vi->ctx, vi->idx, &entity, 1, &removed), "db.idx.vector.unset");
    vi->ends.erase(entity);
    return removed != 0;
}

bool Graph::vector_unset_node(LabelId label, const std::string& attr, u64 node) {
    return unset(const_cast<VectorIndex*>(vector_index(false, label, attr)), node);
}

bool Graph::vector_unset_edge(u64 type, const std::string& attr, u64 edge_id) {
    return unset(const_cast<VectorIndex*>(vector_index(true, type, attr)), edge_id);
}

void Graph::drop_entity_vectors(bool is_edge, std::optional<u64> owner, u64 entity) {
    for (auto& kv : vec_indexes_)
        if (std::get<0>(kv.first) == is_edge && (!owner || std::get<1>(kv.first) == *owner)) unset(kv.second.get(), entity);
}

VectorHits Graph::vector_query(bool is_edge, const std::string& owner_name, const std::string& attr, int64_t k,
                               const float* queries, u64 qn, u64 nq) const {
    if (k <= 0)
        throw std::runtime_error(std::string("Invalid arguments for procedure 'db.idx.vector.") +
                                 (is_edge ? "queryRelationships'" : "queryNodes'"));
    VectorHits out;
    out.offsets.assign(nq + 1, 0);
    const std::optional<u64> owner = is_edge ? type_id(owner_name) : label_id(owner_name);
    const VectorIndex* vi = owner ? vector_index(is_edge, *owner, attr) : nullptr;
    if (!vi) return out;                                   // indexer.rs:525-536: no index, no rows
    if (qn != vi->dim) throw std::runtime_error(dim_mismatch(vi->dim, qn));
    uint64_t count = 0;
    check(fgpu_vecidx_info(vi->idx, nullptr, nullptr, &count), "db.idx.vector.query");
    const u64 kk = std::min<u64>((u64)k, count);
    if (kk == 0 || nq == 0) return out;
    out.ids.resize(nq * kk);
    out.dist.resize(nq * kk);
    uint64_t got = 0;
    check(fgpu_vecidx_knn(vi->ctx, vi->idx, queries, nq, (u64)k, out.ids.data(), out.dist.data(), &got, nullptr),
          "db.idx.vector.query");
    if (got != kk) throw std::runtime_error("db.idx.vector.query: the index changed during the call");
    for (u64 q = 0; q <= nq; ++q) out.offsets[q] = q * kk;
    if (is_edge) {
        out.srcs.resize(out.ids.size());
        out.dsts.resize(out.ids.size());
        for (size_t i = 0; i < out.ids.size(); ++i) {
            const auto& e = vi->ends.at(out.ids[i]);
            out.srcs[i] = e.first;
            out.dsts[i] = e.second;
        }
    }
    return out;
}

}  // namespace falkor
