// tensor.cpp — Tensor: per-relationship-type edge storage with inline edge ids
// (mirrors graph/src/graph/graphblas/tensor.rs; per-pair state diagram at tensor.rs:72-108).
#include <algorithm>
#include <chrono>

#include <unordered_map>

#include "host.hpp"

namespace falkor {

u64 compound_key(u64 src, u64 dst) {
    if ((src >> 32) || (dst >> 32))
        throw GrbError(FGPU_INVALID, "Tensor compound key overflow: src=" + std::to_string(src) +
                                         ", dst=" + std::to_string(dst) + " (each must fit in u32)");
    return (src << 32) | dst;
}

Tensor::Tensor(Context& ctx, u64 nrows, u64 ncols)
    : m_(ctx, Type::UInt64, nrows, ncols),
      dp_(ctx, Type::UInt64, nrows, ncols),
      dm_(ctx, Type::Bool, nrows, ncols),
      mt_(ctx, ncols, nrows) {}

void Tensor::wait_fwd() const {
    if (dp_.is_synced() && dm_.is_synced()) return;
    dp_.resync();
    dm_.resync();
    u64 base = m_.nvals();
    dp_.latch(dp_.fold_decision(should_fold_read, base));
    dm_.latch(dm_.fold_decision(should_fold_read, base));
}

std::optional<u64> Tensor::eff_get(u64 src, u64 dst) const {
    wait_fwd();
    if (auto v = dp_.get(src, dst)) return v;
    if (dm_.nvals() != 0 && dm_.contains(src, dst)) return std::nullopt;
    return m_.get(src, dst);
}

std::vector<u64> Tensor::get(u64 src, u64 dst) const {
    auto v = eff_get(src, dst);
    if (!v) return {};
    if (*v == MULTI_EDGE) {
        auto it = me_.find(compound_key(src, dst));
        return it == me_.end() ? std::vector<u64>{} : it->second;   // ascending
    }
    return {*v};
}

// effective inline value of every pair: dp wins, then m unless dm-masked (three probes for the batch)
static void eff_get_batch(const Matrix& m, const Matrix& dp, const Matrix& dm, const std::vector<u64>& srcs,
                          const std::vector<u64>& dsts, std::vector<uint8_t>& present, std::vector<u64>& vals,
                          std::vector<uint8_t>* masked_out = nullptr, std::vector<uint8_t>* in_dp_out = nullptr,
                          std::vector<uint8_t>* in_m_out = nullptr, std::vector<u64>* m_vals_out = nullptr) {
    std::vector<uint8_t> pd, pm, pk;
    std::vector<u64> vd, vm;
    dp.probe(srcs, dsts, pd, &vd);
    m.probe(srcs, dsts, pm, &vm);
    if (dm.nvals() != 0)
        dm.probe(srcs, dsts, pk, nullptr);
    else
        pk.assign(srcs.size(), 0);
    present.assign(srcs.size(), 0);
    vals.assign(srcs.size(), 0);
    for (size_t k = 0; k < srcs.size(); ++k) {
        if (pd[k]) { present[k] = 1; vals[k] = vd[k]; }
        else if (pk[k]) { present[k] = 0; }
        else if (pm[k]) { present[k] = 1; vals[k] = vm[k]; }
    }
    if (masked_out) *masked_out = pk;
    if (in_dp_out) *in_dp_out = pd;
    if (in_m_out) *in_m_out = pm;
    if (m_vals_out) *m_vals_out = vm;
}

void Tensor::get_batch(const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                       std::vector<std::vector<u64>>& ids) const {
    wait_fwd();
    std::vector<uint8_t> present;
    std::vector<u64> vals;
    eff_get_batch(m_, dp_.layer(), dm_.layer(), srcs, dsts, present, vals);
    ids.assign(srcs.size(), {});
    for (size_t k = 0; k < srcs.size(); ++k) {
        if (!present[k]) continue;
        if (vals[k] == MULTI_EDGE) {
            auto it = me_.find(compound_key(srcs[k], dsts[k]));
            if (it != me_.end()) ids[k] = it->second;
        } else {
            ids[k] = {vals[k]};
        }
    }
}

static void me_insert(std::map<u64, std::vector<u64>>& me, u64 key, u64 id) {
    auto& v = me[key];
    auto it = std::lower_bound(v.begin(), v.end(), id);
    if (it == v.end() || *it != id) v.insert(it, id);
}

void Tensor::set_all_from_slices(const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                                 const std::vector<u64>& ids) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    if (srcs.size() != dsts.size() || srcs.size() != ids.size())
        throw GrbError(FGPU_INVALID, "set_all_from_slices: slices differ in length");
    if (srcs.empty()) return;
    flush();
    dp_.wait();
    dm_.wait();
    // Read phase (tensor.rs:353-421): each edge's placement is decided against the state the layers hold
    // BEFORE this batch; the three probes below read that state for every pair at once.
    std::vector<uint8_t> present, masked, in_dp, in_m;
    std::vector<u64> cur, m_vals;
    eff_get_batch(m_, dp_.layer(), dm_.layer(), srcs, dsts, present, cur, &masked, &in_dp, &in_m, &m_vals);
    constexpr size_t PROMOTED = ~(size_t)0;
    std::unordered_map<u64, size_t> batch;         // pair (compound key) -> index of its pending inline slot, or PROMOTED
    batch.reserve(srcs.size());
    std::vector<u64> w_src, w_dst, w_id;
    std::vector<std::optional<u64>> w_masked;      // committed m value of pairs needing delta reconciliation
    for (size_t k = 0; k < srcs.size(); ++k) {
        const u64 s = srcs[k], d = dsts[k], id = ids[k];
        const u64 key = compound_key(s, d);
        auto it = batch.find(key);
        if (it != batch.end()) {
            if (it->second != PROMOTED) {          // second edge of a pair new in this batch: promote in place
                me_insert(me_, key, w_id[it->second]);
                w_id[it->second] = MULTI_EDGE;
                it->second = PROMOTED;
            }
            me_insert(me_, key, id);
            continue;
        }
        auto committed = [&]() -> std::optional<u64> { return in_m[k] ? std::optional<u64>(m_vals[k]) : std::nullopt; };
        if (present[k] && cur[k] == MULTI_EDGE) {  // already multi-edge: just add the id
            me_insert(me_, key, id);
            batch[key] = PROMOTED;
        } else if (present[k]) {                   // present single edge: promote
            me_insert(me_, key, cur[k]);
            me_insert(me_, key, id);
            batch[key] = PROMOTED;
            w_src.push_back(s); w_dst.push_back(d); w_id.push_back(MULTI_EDGE);
            w_masked.push_back(in_dp[k] ? committed() : std::nullopt);
        } else {                                   // first edge of the pair: inline
            batch[key] = w_id.size();
            w_src.push_back(s); w_dst.push_back(d); w_id.push_back(id);
            w_masked.push_back(masked[k] ? committed() : std::nullopt);
        }
    }
    // Write phase (tensor.rs:429-454).  mt.set(d, s) of every written pair goes out as one set_all: the same
    // per-entry body with its probe of mt's committed base hoisted into one batch.
    {
        std::vector<std::pair<u64, u64>> back(w_src.size());
        for (size_t i = 0; i < w_src.size(); ++i) back[i] = {w_dst[i], w_src[i]};
        mt_.set_all(back, false);
    }
    for (size_t i = 0; i < w_src.size(); ++i) {
        const u64 s = w_src[i], d = w_dst[i], id = w_id[i];
        if (w_masked[i]) {
            dm_.erase(s, d);
            if (*w_masked[i] == id) {              // cancel to clean: committed value restored
                dp_.erase(s, d);
                continue;
            }
        }
        dp_.insert(s, d, id);
    }
}

u64 bulk_clock_ns() {
    return (u64)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Tensor::BuiltBatch {
    Matrix fwd, bwd;               // the batch's UINT64 matrix and its transposed pattern
    EngineBuf<u64> key, off, ids;  // its multi-edge runs, ascending by key
    u64 n_multi;
    u64 st[8];                     // fgpu_edges_build's stats
};

// the build reads nothing of the tensor: an invalid batch throws here, before any layer moved
Tensor::BuiltBatch Tensor::build_batch(const u64* srcs, const u64* dsts, const u64* ids, u64 n, const char* who) const {
    Context& ctx = m_.ctx();
    fgpu_ctx* c = ctx.raw();
    SnapshotRef fwd_h, bwd_h;
    EngineBuf<u64> key(c), off(c), run(c);
    u64 n_multi = 0, st[8] = {0};
    check(fgpu_edges_build(c, m_.nrows(), m_.ncols(), srcs, dsts, ids, n, fwd_h.out(), bwd_h.out(), key.out(), off.out(), run.out(),
                           &n_multi, st),
          who);
    BuiltBatch b{Matrix::adopt(ctx, Type::UInt64, std::move(fwd_h)), Matrix::adopt(ctx, Type::Bool, std::move(bwd_h)), std::move(key),
                 std::move(off), std::move(run), n_multi, {}};
    std::copy(st, st + 8, b.st);
    return b;
}

void Tensor::fold_for_bulk() {
    flush();
    dp_.wait();
    dm_.wait();
    if (dp_.nvals() != 0 || dm_.nvals() != 0) {
        dp_.latch(true);
        dm_.latch(true);
        needs_flush_ = true;
        flush();
    }
    mt_.fold_all();
}

void Tensor::gather_me_rows(const u64* srcs, const u64* dsts, u64 n, std::vector<u64>& key, std::vector<u64>& off, std::vector<u64>& run,
                            std::vector<MeRow>* rows) {
    if (!has_multi_edge()) return;
    std::vector<uint8_t> in_m;
    std::vector<u64> mv;
    m_.probe(std::vector<u64>(srcs, srcs + n), std::vector<u64>(dsts, dsts + n), in_m, &mv);
    for (u64 k = 0; k < n; ++k)
        if (in_m[k] && mv[k] == MULTI_EDGE) key.push_back(compound_key(srcs[k], dsts[k]));
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    size_t kept = 0;
    for (u64 x : key) {
        auto it = me_.find(x);
        if (it == me_.end() || it->second.size() < 2) continue;   // (the device reports the pair when it needs the row)
        key[kept++] = x;
        if (rows) rows->push_back(it);
        run.insert(run.end(), it->second.begin(), it->second.end());
        off.push_back(run.size());
    }
    key.resize(kept);
}

void Tensor::adopt_bases(const Matrix& m, const Matrix& mt) {
    m_ = m;
    mt_ = VersionedMatrix::from_matrix(mt);
}

// the outputs of a device pass over the folded bases; one that changed nothing leaves the bases the snapshots they are
void Tensor::adopt_bases(SnapshotRef&& mo, SnapshotRef&& mto, bool changed) {
    Matrix new_m = Matrix::adopt(m_.ctx(), Type::UInt64, std::move(mo));
    Matrix new_mt = Matrix::adopt(m_.ctx(), Type::Bool, std::move(mto));
    if (changed) adopt_bases(new_m, new_mt);
}

BulkStats Tensor::bulk_insert(const std::vector<u64>& srcs, const std::vector<u64>& dsts, const std::vector<u64>& ids,
                              std::optional<Matrix>* built) {
    if (srcs.size() != dsts.size() || srcs.size() != ids.size())
        throw GrbError(FGPU_INVALID, "bulk_insert: slices differ in length");
    return bulk_insert(srcs.data(), dsts.data(), ids.data(), srcs.size(), built);
}

BulkStats Tensor::bulk_insert(const u64* srcs, const u64* dsts, const u64* ids, u64 n, std::optional<Matrix>* built) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    BulkStats bs;
    if (built) built->reset();
    if (n == 0) return bs;
    Context& ctx = m_.ctx();
    fgpu_ctx* c = ctx.raw();
    u64 t0 = bulk_clock_ns();
    BuiltBatch b = build_batch(srcs, dsts, ids, n, "Tensor::bulk_insert");
    const Matrix &fwd = b.fwd, &bwd = b.bwd;
    bs.phase_ns[0] = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    fold_for_bulk();
    const bool empty = m_.nvals() == 0;
    if (!empty && m_.intersection_nvals(fwd) != 0) {
        // a pair of the batch holds an edge already: its promotion is the edge-by-edge path's
        set_all_from_slices(std::vector<u64>(srcs, srcs + n), std::vector<u64>(dsts, dsts + n), std::vector<u64>(ids, ids + n));
        bs.fallback_edges = n;
        bs.phase_ns[1] = bulk_clock_ns() - t0;
        return bs;
    }
    if (empty) {
        adopt_bases(fwd, bwd);
    } else {
        SnapshotRef merged;
        check(fgpu_mat_merge(c, merged.out(), m_.snapshot(), fwd.snapshot(), nullptr, 0), "Tensor::bulk_insert");
        Matrix new_m = Matrix::adopt(ctx, Type::UInt64, std::move(merged));
        mt_.union_base(bwd);
        m_ = new_m;
    }
    bs.phase_ns[1] = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    for (u64 r = 0; r < b.n_multi; ++r)   // (ascending keys: the hint is the place when the map held nothing above them)
        me_.emplace_hint(me_.end(), b.key.p[r], std::vector<u64>(b.ids.p + b.off.p[r], b.ids.p + b.off.p[r + 1]));
    bs.phase_ns[2] = bulk_clock_ns() - t0;
    bs.device_edges = n;
    bs.distinct_pairs = b.st[0];
    bs.multi_pairs = b.st[1];
    bs.unsorted_runs = b.st[4];
    bs.host_sorted_runs = b.st[6];
    if (built) *built = fwd;
    return bs;
}

AppendStats Tensor::append_bulk(const u64* srcs, const u64* dsts, const u64* ids, u64 n, std::optional<Matrix>* built) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    AppendStats as;
    if (built) built->reset();
    if (n == 0) return as;
    fgpu_ctx* c = m_.ctx().raw();
    u64 t0 = bulk_clock_ns();
    BuiltBatch b = build_batch(srcs, dsts, ids, n, "Tensor::append_bulk");
    const Matrix &fwd = b.fwd, &bwd = b.bwd;
    const EngineBuf<u64> &bkey = b.key, &boff = b.off, &bids = b.ids;
    const u64 n_b = b.n_multi;
    as.phase_ns[0] = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    fold_for_bulk();
    as.edges = n;
    as.distinct_pairs = b.st[0];
    as.multi_pairs = b.st[1];
    as.host_sorted_runs = b.st[6];
    if (m_.nvals() == 0) {
        adopt_bases(fwd, bwd);
        as.phase_ns[1] = bulk_clock_ns() - t0;
        t0 = bulk_clock_ns();
        for (u64 r = 0; r < n_b; ++r)
            me_.insert_or_assign(me_.end(), bkey.p[r], std::vector<u64>(bids.p + boff.p[r], bids.p + boff.p[r + 1]));
        as.me_rows = n_b;
        as.phase_ns[2] = bulk_clock_ns() - t0;
        if (built) *built = fwd;
        return as;
    }
    std::vector<u64> akey, aoff{0}, arun;
    gather_me_rows(srcs, dsts, n, akey, aoff, arun, nullptr);
    SnapshotRef mo, mto;
    EngineBuf<u64> okey(c), ooff(c), oids(c);
    u64 n_o = 0, us[8] = {0};
    // an id already stored on its pair fails here: the layers are folded, the state they hold is what it was
    check(fgpu_edges_union(c, m_.snapshot(), mt_.m().snapshot(), akey.data(), aoff.data(), arun.data(), akey.size(), fwd.snapshot(),
                           bwd.snapshot(), bkey.p, boff.p, bids.p, n_b, mo.out(), mto.out(), okey.out(), ooff.out(), oids.out(), &n_o, us),
          "Tensor::append_bulk");
    adopt_bases(std::move(mo), std::move(mto), true);
    as.phase_ns[1] = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    // b and o ascend by key, one cursor each: a multi-edge pair only the batch names brings its b row, a colliding pair its o row
    auto hint = me_.begin();
    u64 i = 0, j = 0;
    while (i < n_b || j < n_o) {
        const u64 kb = i < n_b ? bkey.p[i] : ~0ull, ko = j < n_o ? okey.p[j] : ~0ull;
        if (ko <= kb) {
            hint = std::next(me_.insert_or_assign(hint, ko, std::vector<u64>(oids.p + ooff.p[j], oids.p + ooff.p[j + 1])));
            ++j;
            if (kb == ko) ++i;
        } else {
            hint = std::next(me_.insert_or_assign(hint, kb, std::vector<u64>(bids.p + boff.p[i], bids.p + boff.p[i + 1])));
            ++i;
        }
        ++as.me_rows;
    }
    as.phase_ns[2] = bulk_clock_ns() - t0;
    as.colliding = us[1];
    as.promoted = us[2];
    as.extended = us[3];
    if (built) *built = fwd;
    return as;
}

std::vector<std::array<u64, 3>> Tensor::detach_nodes(const std::vector<u64>& nodes, const std::unordered_set<u64>& skip_ids,
                                                     DetachCounts* counts) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    std::vector<std::array<u64, 3>> out;
    if (nodes.empty()) return out;
    for (u64 v : nodes)
        if (v >= m_.nrows() || v >= m_.ncols())
            throw GrbError(FGPU_INVALID, "Tensor::detach_nodes: node " + std::to_string(v) + " is outside the tensor");
    fgpu_ctx* c = m_.ctx().raw();
    u64 t0 = bulk_clock_ns();
    fold_for_bulk();
    SnapshotRef mo, mto;
    EngineBuf<u64> rr(c), rc(c), rv(c);
    u64 n_rem = 0, n_out = 0, st[8] = {0};
    check(fgpu_nodes_detach(c, m_.snapshot(), mt_.m().snapshot(), nodes.data(), nodes.size(), 3, mo.out(), mto.out(), rr.out(), rc.out(), rv.out(), &n_rem,
                            &n_out, st),
          "Tensor::detach_nodes");
    adopt_bases(std::move(mo), std::move(mto), n_rem != 0);   // (nothing incident: nothing changed)
    if (counts) counts->phase_ns[0] += bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    // the reference's order (graph.rs:2405-2427): per node of D ascending its out edges, then its in edges.  The out segment
    // ascends in (src, dst) and the in segment in (dst, src), so one cursor on each walks the nodes in step
    out.reserve(n_rem);
    u64 removed = 0, multi = 0;
    auto emit = [&](u64 k) {
        const u64 s = rr.p[k], d = rc.p[k], v = rv.p[k];
        if (v != MULTI_EDGE) {
            ++removed;
            if (skip_ids.empty() || !skip_ids.count(v)) out.push_back({v, s, d});
            else if (counts) counts->skipped.push_back(v);
            return;
        }
        auto it = me_.find(compound_key(s, d));
        if (it == me_.end()) return;
        ++multi;
        for (u64 id : it->second) {   // ascending
            ++removed;
            if (skip_ids.empty() || !skip_ids.count(id)) out.push_back({id, s, d});
            else if (counts) counts->skipped.push_back(id);
        }
        me_.erase(it);
    };
    u64 i = 0, j = n_out;
    while (i < n_out || j < n_rem) {
        const u64 a = i < n_out ? rr.p[i] : ~0ull, b = j < n_rem ? rc.p[j] : ~0ull;
        const u64 node = std::min(a, b);
        while (i < n_out && rr.p[i] == node) emit(i++);
        while (j < n_rem && rc.p[j] == node) emit(j++);
    }
    if (counts) {
        counts->removed += removed;
        counts->multi_pairs += multi;
        counts->phase_ns[1] += bulk_clock_ns() - t0;
    }
    return out;
}

std::vector<std::pair<u64, u64>> Tensor::remove_all(const std::vector<std::array<u64, 3>>& rels) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    std::vector<std::pair<u64, u64>> emptied;
    if (rels.empty()) return emptied;
    flush();
    Context& ctx = m_.ctx();
    if (!has_multi_edge()) {
        // Fast path (tensor.rs:473-505): every edge is the inline value of its pair
        wait_fwd();
        std::vector<u64> mr, mc;
        for (auto& r : rels) { mr.push_back(r[1]); mc.push_back(r[2]); }
        Matrix m_mask(ctx, Type::Bool, m_.nrows(), m_.ncols());
        m_mask.build(mr, mc);
        Matrix mt_mask(ctx, Type::Bool, m_.ncols(), m_.nrows());
        mt_mask.build(mc, mr);
        dm_.tombstone_masked(m_mask, m_);
        dp_.remove_all(m_mask);
        mt_.remove_mask(mt_mask);
        for (auto& r : rels) emptied.push_back({r[1], r[2]});
        return emptied;
    }
    // Slow path (tensor.rs:507-655): read phase replays each touched pair's transitions, write phase applies
    wait_fwd();
    struct Plan {
        enum Kind { Multi, Single, Emptied, Absent } kind = Absent;
        std::vector<u64> ids;   // Multi: ids still in the me row
        u64 id = 0;             // Single
        bool demoted = false;
    };
    std::vector<std::pair<u64, u64>> order;
    std::map<std::pair<u64, u64>, Plan> plans;
    {   // effective state of every distinct pair, one batch of probes
        std::vector<u64> ps, pd;
        for (auto& r : rels)
            if (plans.emplace(std::make_pair(r[1], r[2]), Plan{}).second) { ps.push_back(r[1]); pd.push_back(r[2]); }
        std::vector<uint8_t> present;
        std::vector<u64> vals;
        eff_get_batch(m_, dp_.layer(), dm_.layer(), ps, pd, present, vals);
        for (size_t k = 0; k < ps.size(); ++k) {
            Plan& p = plans[{ps[k], pd[k]}];
            if (!present[k]) p.kind = Plan::Absent;
            else if (vals[k] == MULTI_EDGE) {
                p.kind = Plan::Multi;
                auto it = me_.find(compound_key(ps[k], pd[k]));
                if (it != me_.end()) p.ids = it->second;
            } else { p.kind = Plan::Single; p.id = vals[k]; }
            order.push_back({ps[k], pd[k]});
        }
    }
    std::vector<std::pair<u64, u64>> me_del;   // (key, id)
    for (auto& r : rels) {
        const u64 id = r[0], src = r[1], dst = r[2];
        const u64 key = compound_key(src, dst);
        Plan& p = plans[{src, dst}];
        if (p.kind == Plan::Multi) {
            auto it = std::lower_bound(p.ids.begin(), p.ids.end(), id);
            if (it == p.ids.end() || *it != id) continue;   // unknown id
            p.ids.erase(it);
            me_del.push_back({key, id});
            if (p.ids.size() == 1) {                        // demote: survivor returns inline
                u64 last = p.ids[0];
                me_del.push_back({key, last});
                p.kind = Plan::Single;
                p.id = last;
                p.demoted = true;
                p.ids.clear();
            }
        } else if (p.kind == Plan::Single && p.id == id) {
            p.kind = Plan::Emptied;
            emptied.push_back({src, dst});
        }
    }
    // Write phase: me first, then the forward / backward layers
    for (auto& kd : me_del) {
        auto it = me_.find(kd.first);
        if (it == me_.end()) continue;
        auto pos = std::lower_bound(it->second.begin(), it->second.end(), kd.second);
        if (pos != it->second.end() && *pos == kd.second) it->second.erase(pos);
        if (it->second.empty()) me_.erase(it);
    }
    std::vector<std::array<u64, 3>> dp_set;
    {   // committed values of the touched pairs (m is never pending): one probe
        std::vector<u64> ps, pd;
        for (auto& pr : order) { ps.push_back(pr.first); pd.push_back(pr.second); }
        std::vector<uint8_t> in_m;
        std::vector<u64> mv;
        m_.probe(ps, pd, in_m, &mv);
        for (size_t k = 0; k < order.size(); ++k) {
            const u64 src = order[k].first, dst = order[k].second;
            const Plan& p = plans[order[k]];
            if (p.kind == Plan::Emptied) {
                dp_.erase(src, dst);
                if (in_m[k]) dm_.insert(src, dst);
                mt_.remove(dst, src);
            } else if (p.kind == Plan::Single && p.demoted) {
                if (in_m[k] && mv[k] == p.id) dp_.erase(src, dst);   // cancel to clean
                else dp_set.push_back({src, dst, p.id});
            }
        }
    }
    for (auto& t : dp_set) dp_.insert(t[0], t[1], t[2]);
    return emptied;
}

const fgpu_multi* Tensor::multi_table() const {
    if (me_.empty()) return nullptr;
    // readers of one const Graph run on several threads (threadpool.rs:89-128): the first of them builds the table
    static std::mutex build_mu;
    std::lock_guard<std::mutex> lock(build_mu);
    if (multi_) return multi_->get();
    std::vector<u64> key, off{0}, run;
    key.reserve(me_.size());
    for (auto& kv : me_) {
        if (kv.second.size() < 2) continue;   // (an inline pair needs no row)
        key.push_back(kv.first);
        run.insert(run.end(), kv.second.begin(), kv.second.end());
        off.push_back(run.size());
    }
    auto t = std::make_shared<MultiRef>();
    check(fgpu_multi_new(m_.ctx().raw(), key.data(), off.data(), run.data(), key.size(), t->out()), "Tensor::multi_table");
    multi_ = std::move(t);
    return multi_->get();
}

void Tensor::contains_batch(const std::vector<u64>& srcs, const std::vector<u64>& dsts, std::vector<uint8_t>& present) const {
    wait_fwd();
    std::vector<u64> vals;
    eff_get_batch(m_, dp_.layer(), dm_.layer(), srcs, dsts, present, vals);
}

std::vector<std::pair<u64, u64>> Tensor::remove_bulk(const u64* srcs, const u64* dsts, const u64* ids, u64 n, RemoveCounts* counts) {
    multi_.reset();   // me_ may change: the resident table is rebuilt on the next batch that needs it
    std::vector<std::pair<u64, u64>> emptied;
    if (counts) counts->hit.assign(n, 0);
    if (n == 0) return emptied;
    for (u64 k = 0; k < n; ++k)
        if (srcs[k] >= m_.nrows() || dsts[k] >= m_.ncols())
            throw GrbError(FGPU_INVALID, "Tensor::remove_bulk: edge (" + std::to_string(srcs[k]) + ", " + std::to_string(dsts[k]) +
                                             ") is outside the tensor");
    fgpu_ctx* c = m_.ctx().raw();
    u64 t0 = bulk_clock_ns();
    fold_for_bulk();
    const u64 fold_ns = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    std::vector<u64> key, off{0}, run;
    std::vector<MeRow> rows;
    gather_me_rows(srcs, dsts, n, key, off, run, &rows);
    std::vector<uint8_t> taken(run.size(), 0), hit_local;
    std::vector<uint8_t>& hit = counts ? counts->hit : hit_local;
    hit.assign(n, 0);
    const u64 gather_ns = bulk_clock_ns() - t0;
    t0 = bulk_clock_ns();
    SnapshotRef mo, mto;
    EngineBuf<u64> er(c), ec(c);
    u64 n_emp = 0, st[8] = {0};
    check(fgpu_edges_remove(c, m_.snapshot(), mt_.m().snapshot(), srcs, dsts, ids, n, key.data(), off.data(), run.data(), key.size(),
                            mo.out(), mto.out(), hit.data(), taken.data(), er.out(), ec.out(), &n_emp, st),
          "Tensor::remove_bulk");
    adopt_bases(std::move(mo), std::move(mto), st[0] != 0);   // (nothing hit: nothing changed)
    emptied.reserve(n_emp);
    for (u64 k = 0; k < n_emp; ++k) emptied.push_back({er.p[k], ec.p[k]});
    const u64 device_ns = fold_ns + (bulk_clock_ns() - t0);
    t0 = bulk_clock_ns();
    for (size_t r = 0; r < rows.size(); ++r) {
        std::vector<u64>& v = rows[r]->second;
        const uint8_t* tk = taken.data() + off[r];
        size_t left = 0;
        for (size_t j = 0; j < v.size(); ++j)
            if (!tk[j]) v[left++] = v[j];
        if (left == v.size()) continue;
        if (left < 2) me_.erase(rows[r]);   // demoted (the survivor is inline in m now) or emptied
        else v.resize(left);
    }
    if (counts) {
        counts->hits = st[0];
        counts->removed = (n_emp - st[2]) + (u64)std::count(taken.begin(), taken.end(), (uint8_t)1);
        counts->emptied_multi = st[2];
        counts->demoted = st[3];
        counts->phase_ns[0] += gather_ns;
        counts->phase_ns[1] += device_ns;
        counts->phase_ns[2] += bulk_clock_ns() - t0;
    }
    return emptied;
}

void Tensor::resize(u64 nrows, u64 ncols) {
    if (nrows < m_.nrows() || ncols < m_.ncols()) flush();
    m_.wait();
    dp_.wait();
    dm_.wait();
    m_ = m_.grown(nrows, ncols);   // also the shrink path: entries past the new dims are dropped
    dp_.replace(dp_.nvals() > 0 ? dp_.layer().grown(nrows, ncols) : Matrix(m_.ctx(), Type::UInt64, nrows, ncols));
    dm_.replace(dm_.nvals() > 0 ? dm_.layer().grown(nrows, ncols) : Matrix(m_.ctx(), Type::Bool, nrows, ncols));
    mt_.resize(ncols, nrows);
}

void Tensor::flush() {
    if (needs_flush_) {
        m_.wait();
        dp_.wait();
        dm_.wait();
        bool fold_dp = dp_.take_fold();
        bool fold_dm = dm_.take_fold();
        if (fold_dp || fold_dm) {
            u64 nr = m_.nrows(), nc = m_.ncols();
            Matrix new_m(m_.ctx(), Type::UInt64, nr, nc);
            if (fold_dp && fold_dm)
                new_m.element_wise_add(&dm_.layer(), &m_, &dp_.layer(), Descriptor::RC);  // dp wins on shadowed pairs
            else if (fold_dp)
                new_m.element_wise_add(nullptr, &m_, &dp_.layer(), Descriptor::None);
            else
                new_m.select(dm_.layer(), m_);
            new_m.wait();
            m_ = new_m;
            if (fold_dp) dp_.clear(nr, nc);
            if (fold_dm) dm_.clear(nr, nc);
        }
        needs_flush_ = false;
    }
    mt_.flush();
}

void Tensor::fold_oversized() {
    u64 base = m_.nvals();
    bool odp = delta_dominates_base(dp_.count(), base);
    bool odm = delta_dominates_base(dm_.count(), base);
    if (odp || odm) {
        dp_.latch(odp);
        dm_.latch(odm);
        needs_flush_ = true;
        flush();
    }
    mt_.fold_oversized();
}

Matrix Tensor::extract() const {
    wait_fwd();
    SnapshotRef o;
    check(fgpu_mat_merge_pattern(m_.ctx().raw(), o.out(), m_.snapshot(), dp_.layer().snapshot(), dm_.layer().snapshot(), 0),
          "Tensor::extract");
    return Matrix::adopt(m_.ctx(), Type::Bool, std::move(o));
}

Tensor Tensor::dup() const {
    u64 base = m_.nvals();
    bool fold_dp = dp_.fold_decision(should_fold, base);
    bool fold_dm = dm_.fold_decision(should_fold, base);
    Tensor t(*this);
    t.m_ = m_.dup();
    t.dp_ = dp_.new_version(fold_dp);
    t.dm_ = dm_.new_version(fold_dm);
    t.mt_ = mt_.dup();
    t.needs_flush_ = fold_dp || fold_dm;
    return t;
}

std::vector<Entry> Tensor::structural_iter(u64 min_row, u64 max_row) const {
    wait_fwd();
    auto out = merge_layers(m_.iter(min_row, max_row), dp_.layer().iter(min_row, max_row),
                            dm_.layer().iter(min_row, max_row));
    for (auto& e : out) e.val = 1;
    return out;
}

std::vector<Entry> Tensor::iter_edges() const {
    wait_fwd();
    auto fwd = merge_layers(m_.iter(0, ~0ull), dp_.layer().iter(0, ~0ull), dm_.layer().iter(0, ~0ull));
    std::vector<Entry> out;
    for (auto& e : fwd)
        if (e.val != MULTI_EDGE) out.push_back(e);
    for (auto& kv : me_)
        for (u64 id : kv.second) out.push_back(Entry{kv.first >> 32, kv.first & 0xFFFFFFFFull, id});
    return out;
}

u64 Tensor::edge_count() const {
    wait_fwd();
    u64 shadow = dp_.nvals() == 0 ? 0 : dp_.layer().intersection_nvals(m_);
    u64 me_nvals = 0;
    for (auto& kv : me_) me_nvals += kv.second.size();
    return m_.nvals() + dp_.nvals() - dm_.nvals() - shadow - multi_pairs() + me_nvals;
}

}  // namespace falkor
