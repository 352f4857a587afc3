// spath_batch.hip — fgpu_shortest_path_batch: the reference's shortestPath() (runtime/eval.rs:1386-1513, bfs_shortest_path) for
// a whole batch of (src, dst) queries.  The reference returns ONE particular path, fixed by the order of its frontiers, by the
// side it grows (the one with fewer frontier vertices) and by the first discoverer of every vertex; include/fgpu.h restates
// the rules.  fgpu_shortest_dag_batch keeps none of the three (its vertices go to whichever lane wins an atomicCAS), so this is
// a search of its own: an order-preserving bidirectional BFS, deterministic to the vertex, batched as spdag_batch.hip batches
// its queries — a GROUP of up to `slots` queries advances in lock-step rounds and shares each round's launches and its one
// counter read-back (spath_plan.hpp plans the rounds).
//
// State of a group.  Every (slot, side) has a dense 64-bit claim word and a 32-bit parent per vertex: 24 nrows bytes per slot,
// all that is sized by slots x nrows.  A claim word holds (depth << 32) | key, all ones while the vertex is outside the ball.
// The frontiers live in one pool of vertex ids in segments the planner reserves; three per-entry arrays (winner flags, their
// scan, the claimed vertex) grow with the entries walked.
// A round is: the descriptor table uploaded (SpDesc: slot, side, frontier slice, entry total, depth, output segment),
// spb_lens_kernel writing the row length of every frontier vertex of every descriptor into one concatenated list, one scan_u32
// over it, then a lane per entry e — key = e's position in its descriptor's walk, frontier order then ascending column — in
//   spb_claim_kernel:   atomicMin of (depth << 32) | key into the claim word of the entry's column.  A word that already holds
//                       a smaller depth keeps it: the vertex was visited earlier;
//   spb_resolve_kernel: the lane whose value the word now holds is the vertex' first discoverer: it stores the parent (plain
//                       store) and flags its entry; if the other ball holds the vertex it is a meeting candidate:
//                       atomicMin of (other depth << 32) | key into the slot's meeting word;
//   scan_u32 over the flags, and
//   spb_place_kernel:   winners go to the output segment at their rank among the descriptor's winners — key order, so the next
//                       frontier is the reference's (an append by ballot and atomicAdd would reorder it across wavefronts);
//                       the winner behind the meeting word's key stores the meeting vertex; the last entry's lane stores the
//                       count; the row lengths of the winners are summed per wavefront into the side's entry counter.
// Meeting candidates are placed like the other winners: only a query's LAST level has any, its frontier is never walked, and
// the reset finds every claimed vertex in a segment.  After the rounds one launch walks the parents of every found query
// (spb_walk_kernel, a lane per query), and between groups spb_reset_kernel restores the claim words by walking the segments.
//
// The concurrency rules are those of spdag.hip: atomics only on the claim words of a query's expanding side (one side per
// query and round), on the meeting words and on counters; the other side's words are read-only inside a launch; parents,
// flags, pool slots and counts are written once with plain stores and read by LATER launches; nothing polls or spins; no
// inline assembly.  Nothing is cached on the matrices; the call runs on the calling thread's lane.  No LDS.
#include <vector>

#include "algo.hpp"
#include "spath_plan.hpp"

namespace fgpu {

using spb::SpCtl;
using spb::SpDesc;
using spb::SpWalk;

constexpr u64 SPB_UNSET = ~0ull;

// the last descriptor j with d[j].ebase <= x / d[j].cbase <= x (both ascend from 0; every descriptor has rows and entries)
__device__ __forceinline__ u32 spb_by_entry(const SpDesc* __restrict__ d, u32 nd, u32 x) {
    u32 lo = 0, hi = nd;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (d[mid].ebase <= x) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u32 spb_by_row(const SpDesc* __restrict__ d, u32 nd, u32 x) {
    u32 lo = 0, hi = nd;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (d[mid].cbase <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// entry e of the round: its descriptor, the frontier vertex u whose row holds it, its column v, its key and claim value
struct SpbEntry {
    u32 j, u, v, key;
    u64 val;
};
__device__ __forceinline__ SpbEntry spb_entry(const CsrView& f, const CsrView& b, const SpDesc* __restrict__ desc, u32 nd,
                                              const u32* __restrict__ off, const u32* __restrict__ pool, u32 e) {
    SpbEntry t;
    t.j = spb_by_entry(desc, nd, e);
    const SpDesc& d = desc[t.j];
    const u32 i = d.cbase + csr_row_of(off + d.cbase, d.cnt, e);
    const CsrView& m = d.side ? b : f;
    t.u = pool[d.qbase + (i - d.cbase)];
    const u32 at = m.rowptr[t.u] + (e - off[i]);
    t.v = at < m.rowptr[t.u + 1] ? m.colidx[at] : spb::NONE;   // (NONE: see the callers)
    t.key = e - d.ebase;
    t.val = ((u64)d.level << 32) | t.key;
    return t;
}

// a lane per query of the group: pool[2 j] = src and pool[2 j + 1] = dst are in place; the seeds' words and the entry counters
__global__ void spb_seed_kernel(const u32* __restrict__ frp, const u32* __restrict__ brp, const u32* __restrict__ pool, u32 gn,
                                u64* __restrict__ word, u32 n, SpCtl* __restrict__ ctl) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= gn) return;
    const u32 src = pool[2 * j], dst = pool[2 * j + 1];
    ctl[j].ent[0] = frp[src + 1] - frp[src];
    ctl[j].ent[1] = brp[dst + 1] - brp[dst];
    if (src == dst) return;   // (no path: the query never enters a round and leaves no word to reset)
    word[(size_t)(2 * j) * n + src] = 0;
    word[(size_t)(2 * j + 1) * n + dst] = 0;
}

// lcat[i] = the row length of the i-th frontier vertex of the round, in the matrix its descriptor's side reads
__global__ __launch_bounds__(256) void spb_lens_kernel(const SpDesc* __restrict__ desc, u32 nd, u32 rows, const u32* __restrict__ pool,
                                                      const u32* __restrict__ frp, const u32* __restrict__ brp,
                                                      u32* __restrict__ lcat) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        const u32 j = spb_by_row(desc, nd, i);
        const u32 v = pool[desc[j].qbase + (i - desc[j].cbase)];
        const u32* rp = desc[j].side ? brp : frp;
        lcat[i] = rp[v + 1] - rp[v];
    }
}

__global__ __launch_bounds__(256) void spb_claim_kernel(CsrView f, CsrView b, const SpDesc* __restrict__ desc, u32 nd, u32 total,
                                                       const u32* __restrict__ off, const u32* __restrict__ pool, u64* word, u32 n) {
    for (u32 e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const SpbEntry t = spb_entry(f, b, desc, nd, off, pool, e);
        if (t.v >= n) continue;   // (never in a correct run: the planner's entry totals are the device's own row sums)
        u64* w = word + (size_t)(2 * desc[t.j].slot + desc[t.j].side) * n + t.v;
        // (a stale read can only be LARGER than the word: it never skips a claim that would win)
        if ((*w >> 32) >= desc[t.j].level) atomicMin((unsigned long long*)w, (unsigned long long)t.val);
    }
}

__global__ __launch_bounds__(256) void spb_resolve_kernel(CsrView f, CsrView b, const SpDesc* __restrict__ desc, u32 nd, u32 total,
                                                         const u32* __restrict__ off, const u32* __restrict__ pool,
                                                         const u64* __restrict__ word, u32* __restrict__ par, u32 n,
                                                         u32* __restrict__ flag, u32* __restrict__ cv, SpCtl* ctl) {
    for (u32 e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const SpbEntry t = spb_entry(f, b, desc, nd, off, pool, e);
        const u32 slot = desc[t.j].slot, side = desc[t.j].side;
        const size_t mine = (size_t)(2 * slot + side) * n, other = (size_t)(2 * slot + (side ^ 1u)) * n;
        const bool won = t.v < n && word[mine + t.v] == t.val;
        flag[e] = won ? 1u : 0u;
        if (!won) continue;
        cv[e] = t.v;
        par[mine + t.v] = t.u;
        const u64 ow = word[other + t.v];
        if (ow != SPB_UNSET) {
            atomicMin((unsigned long long*)&ctl[slot].meet, (unsigned long long)((ow & 0xFFFFFFFF00000000ull) | t.key));
            atomicAdd(&ctl[slot].cand, 1u);
        }
    }
}

// the sum of x over the lanes of the wavefront, in every lane
__device__ __forceinline__ u64 spb_wave_sum(u64 x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// pos[] is the exclusive prefix of flag[] over the round: winner e of descriptor d is its (pos[e] - pos[d.ebase])-th
__global__ __launch_bounds__(256) void spb_place_kernel(CsrView f, CsrView b, const SpDesc* __restrict__ desc, u32 nd, u32 total,
                                                       const u32* __restrict__ flag, const u32* __restrict__ pos,
                                                       const u32* __restrict__ cv, u32* __restrict__ pool, SpCtl* ctl) {
    const u32 lane = lane_id();
    for (u32 e0 = blockIdx.x * 256u; e0 < total; e0 += gridDim.x * 256u) {   // (whole waves stay in the loop: the shuffles)
        const u32 e = e0 + threadIdx.x;
        const bool act = e < total;
        u32 j = 0, deg = 0;
        if (act) {
            j = spb_by_entry(desc, nd, e);
            const SpDesc& d = desc[j];
            SpCtl* c = ctl + d.slot;
            const u32 won = flag[e], rank = pos[e] - pos[d.ebase];
            if (won) {
                const u32 v = cv[e];
                if (rank < d.ocap) pool[d.obase + rank] = v;
                const u32* rp = d.side ? b.rowptr : f.rowptr;
                deg = rp[v + 1] - rp[v];
                if (c->meet != SPB_UNSET && (u32)c->meet == e - d.ebase) c->meetv = v;
            }
            if (e == d.ebase + d.total - 1) c->cnt[d.side] = rank + won;
        }
        for (u64 todo = __ballot(act); todo;) {   // once per descriptor present in the wavefront
            const u32 jl = __shfl(j, __ffsll((unsigned long long)todo) - 1, 64);
            const bool in = act && j == jl;
            todo &= ~__ballot(in);
            const u64 ents = spb_wave_sum(in ? deg : 0u);
            if (lane == 0 && ents) atomicAdd((unsigned long long*)&ctl[desc[jl].slot].ent[desc[jl].side], (unsigned long long)ents);
        }
    }
}

// a lane per found query: the forward parents from the meeting vertex back to src, written in reverse, then the backward
// parents on to dst: length + 1 node ids
__global__ void spb_walk_kernel(const SpWalk* __restrict__ walk, u32 nw, const u64* __restrict__ word, const u32* __restrict__ par,
                                u32 n, u64* __restrict__ nodes) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nw) return;
    const SpWalk w = walk[k];
    const size_t fw = (size_t)(2 * w.slot) * n, bw = (size_t)(2 * w.slot + 1) * n;
    u64* out = nodes + w.off;
    if (w.meet >= n) return;
    u32 at =(u32)(word[fw + w.meet] >> 32);
    if (at > w.length) return;   // (never in a correct run: the two depths add up to the length)
    const u32 mid = at;
    u32 cur = w.meet;
    out[at] = cur;
    while (at > 0 && cur < n) {
        cur = par[fw + cur];
        out[--at] = cur;
    }
    cur = w.meet;
    for (at = mid; at < w.length && cur < n;) {
        cur = par[bw + cur];
        out[++at] = cur;
    }
}

// the claim words a group set go back to "unset": a lane per vertex of every segment
__global__ __launch_bounds__(256) void spb_reset_kernel(const SpDesc* __restrict__ desc, u32 nd, u32 rows, const u32* __restrict__ pool,
                                                       u64* __restrict__ word, u32 n) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        const u32 j = spb_by_row(desc, nd, i);
        const u32 v = pool[desc[j].qbase + (i - desc[j].cbase)];
        word[(size_t)(2 * desc[j].slot + desc[j].side) * n + v] = SPB_UNSET;
    }
}

// the device state of a call and the launches of a round
struct SpathBatch {
    fgpu_ctx* ctx;
    const fgpu_mat* F;
    const fgpu_mat* B;
    u32 n = 0, slots = 0;
    DevBuf<u64> word;
    DevBuf<u32> par, pool, lcat, off, flag, pos, cv;
    DevBuf<SpCtl> ctl;
    DevBuf<SpDesc> desc;
    std::vector<SpCtl> h;   // as last read: the counters of the group's slots

    // b holds at least `need` items, its first `keep` preserved (the old block goes back to the lane's pool in stream order)
    template <class T>
    fgpu_info grow(DevBuf<T>& b, u64 need, u64 keep) {
        if (need <= b.n && b.p) return FGPU_OK;
        u64 cap = b.n ? b.n : 4096;
        while (cap < need) cap *= 2;
        DevBuf<T> nb;
        FGPU_TRY(nb.alloc(ctx, (size_t)cap));
        if (keep) FGPU_HIP(hipMemcpyAsync(nb.p, b.p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream()));
        b = std::move(nb);
        return FGPU_OK;
    }

    fgpu_info upload(const std::vector<SpDesc>& d) {
        FGPU_TRY(grow(desc, d.size(), 0));
        return ctx->h2d(desc.p, d.data(), d.size() * sizeof(SpDesc));
    }

    fgpu_info read(u32 gn) {
        h.resize(gn);
        return ctx->d2h(h.data(), ctl.p, (size_t)gn * sizeof(SpCtl));
    }

    // the launches of one planned round; pool_kept: what the pool held before the planner reserved for it
    fgpu_info run(const spb::Round& rd, u64 pool_kept, u64 pool_used) {
        hipStream_t st = ctx->stream();
        const u32 nd = (u32)rd.desc.size(), rows = (u32)rd.rows, total = (u32)rd.entries;
        FGPU_TRY(grow(pool, pool_used, pool_kept));
        FGPU_TRY(grow(lcat, rows, 0));
        FGPU_TRY(grow(off, rows, 0));
        FGPU_TRY(grow(flag, total, 0));
        FGPU_TRY(grow(pos, total, 0));
        FGPU_TRY(grow(cv, total, 0));
        FGPU_TRY(upload(rd.desc));
        const SpDesc* dp = desc.p;
        const dim3 grid(capped_grid(ctx, total, 256, 8));
        FGPU_TRY(launch(spb_lens_kernel, dim3(capped_grid(ctx, rows, 256, 4)), dim3(256), 0, st, dp, nd, rows, (const u32*)pool.p,
                        (const u32*)F->rowptr, (const u32*)B->rowptr, lcat.p));
        FGPU_TRY(scan_u32(ctx, lcat.p, off.p, rows, nullptr));
        FGPU_TRY(launch(spb_claim_kernel, grid, dim3(256), 0, st, view_of(F), view_of(B), dp, nd, total, (const u32*)off.p,
                        (const u32*)pool.p, word.p, n));
        FGPU_TRY(launch(spb_resolve_kernel, grid, dim3(256), 0, st, view_of(F), view_of(B), dp, nd, total, (const u32*)off.p,
                        (const u32*)pool.p, (const u64*)word.p, par.p, n, flag.p, cv.p, ctl.p));
        FGPU_TRY(scan_u32(ctx, flag.p, pos.p, total, nullptr));
        FGPU_TRY(launch(spb_place_kernel, grid, dim3(256), 0, st, view_of(F), view_of(B), dp, nd, total, (const u32*)flag.p,
                        (const u32*)pos.p, (const u32*)cv.p, pool.p, ctl.p));
        return FGPU_OK;
    }
};

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_shortest_path_batch(fgpu_ctx* ctx, const fgpu_mat* F, const fgpu_mat* B, const uint64_t* src,
                                              const uint64_t* dst, uint64_t count, int64_t max_hops, uint32_t slots, int64_t* length,
                                              uint64_t* node_off, uint64_t** nodes, uint64_t* stats) {
    const char* who = "fgpu_shortest_path_batch";
    FGPU_REQUIRE(ctx && F && length && node_off && nodes && (count == 0 || (src && dst)), FGPU_NULL_POINTER, "%s: NULL argument", who);
    FGPU_TRY(check_adjacency(who, F, B));
    FGPU_REQUIRE(slots <= spb::SLOTS_MAX, FGPU_INVALID, "%s: slots %u exceeds %u", who, slots, spb::SLOTS_MAX);
    const u32 n = (u32)F->nrows;
    if (n)
        for (u64 i = 0; i < count; ++i)
            FGPU_REQUIRE(src[i] < F->nrows && dst[i] < F->nrows, FGPU_OUT_OF_BOUNDS, "%s: %s of query %llu out of range", who,
                         src[i] < F->nrows ? "dst" : "src", (unsigned long long)i);
    FGPU_REQUIRE(F->nnz < 0xFFFFFFFFull && (!B || B->nnz < 0xFFFFFFFFull), FGPU_INVALID, "%s: too many entries", who);
    *nodes = nullptr;
    for (u64 i = 0; i < count; ++i) length[i] = -1;
    for (u64 i = 0; i <= count; ++i) node_off[i] = 0;
    if (stats)
        for (u64 i = 0; i < count; ++i) {
            memset(stats + 8 * i, 0, 8 * sizeof(uint64_t));
            stats[8 * i + 5] = ~0ull;
        }
    if (count == 0 || n == 0 || max_hops == 0) return FGPU_OK;
    if (F->nnz == 0) {   // the one level of a search over nothing: forward, from a seed without entries
        if (stats)
            for (u64 i = 0; i < count; ++i)
                if (src[i] != dst[i]) stats[8 * i] = 1;
        return FGPU_OK;
    }
    DenseInputs in;
    FGPU_TRY(in.a(ctx, F));
    if (!B) {   // a missing transpose: built once for the call, released with the guard
        FGPU_TRY(mat_transpose_pattern(ctx, &in.dAt.m, F));
        B = in.dAt.get();
    }
    FGPU_TRY(in.at(ctx, B));
    hipStream_t st = ctx->stream();

    SpathBatch b;
    b.ctx = ctx;
    b.F = F;
    b.B = B;
    b.n = n;
    b.slots = spb::derive_slots(count, n, slots);
    const size_t S = b.slots;
    FGPU_TRY(b.word.alloc(ctx, S * 2 * n));
    FGPU_TRY(b.par.alloc(ctx, S * 2 * n));
    FGPU_TRY(b.ctl.alloc(ctx, S));
    FGPU_HIP(hipMemsetAsync(b.word.p, 0xFF, S * 2 * n * sizeof(u64), st));

    std::vector<u64> hnodes;   // the paths of the groups done so far
    std::vector<spb::Query> qs;
    std::vector<spb::Seg> segs;
    std::vector<u32> seeds;
    std::vector<SpCtl> ctl0;
    std::vector<SpWalk> walks;
    DevBuf<SpWalk> dwalk;
    spb::Round rd;
    const u64 groups = spb::group_count(count, b.slots);
    for (u64 g = 0; g < groups; ++g) {
        u64 first;
        u32 gn;
        spb::group_range(count, b.slots, g, &first, &gn);
        spb::Pool pool;
        segs.clear();
        qs.resize(gn);
        seeds.resize(2 * (size_t)gn);
        ctl0.assign(gn, SpCtl{spb::NO_MEET, {0, 0}, {0, 0}, 0, spb::NONE});
        for (u32 j = 0; j < gn; ++j) {
            spb::seed_query(qs[j], j, (u32)src[first + j], (u32)dst[first + j]);
            seeds[2 * j] = qs[j].src;
            seeds[2 * j + 1] = qs[j].dst;
            if (qs[j].src == qs[j].dst) continue;
            segs.push_back(spb::Seg{j, 0, 2 * j, 1});
            segs.push_back(spb::Seg{j, 1, 2 * j + 1, 1});
        }
        pool.reserve(2 * (u64)gn);
        FGPU_TRY(b.grow(b.pool, pool.used, 0));
        FGPU_TRY(ctx->h2d(b.pool.p, seeds.data(), seeds.size() * sizeof(u32)));
        FGPU_TRY(ctx->h2d(b.ctl.p, ctl0.data(), ctl0.size() * sizeof(SpCtl)));
        FGPU_TRY(launch(spb_seed_kernel, dim3((gn + 63) / 64), dim3(64), 0, st, (const u32*)F->rowptr, (const u32*)B->rowptr,
                        (const u32*)b.pool.p, gn, b.word.p, n, b.ctl.p));
        FGPU_TRY(b.read(gn));
        for (u32 j = 0; j < gn; ++j) spb::seed_degrees(qs[j], b.h[j].ent[0], b.h[j].ent[1]);

        // ---- the searches, a level of every live query per round ----
        for (;;) {
            const u64 kept = pool.used;
            FGPU_REQUIRE(spb::plan_search(qs, max_hops, n, pool, rd), FGPU_INVALID, "%s: the frontiers of a group outgrew 2^32", who);
            if (rd.empty()) break;
            FGPU_TRY(b.run(rd, kept, pool.used));
            FGPU_TRY(b.read(gn));
            FGPU_REQUIRE(spb::apply_search(qs, rd, b.h.data(), segs), FGPU_DEVICE, "%s: a frontier outgrew its segment", who);
        }

        // ---- the paths of the found queries, out ----
        walks.clear();
        u64 K = 0;
        for (const spb::Query& q : qs) {
            if (stats) spb::fill_stats(q, stats + 8 * (first + q.slot));
            if (q.state != spb::FOUND) continue;
            length[first + q.slot] = (int64_t)q.length;
            node_off[first + q.slot + 1] = (u64)q.length + 1;   // (counts for now; the prefix is taken at the end)
            walks.push_back(SpWalk{q.slot, q.meetv, q.length, 0, K});
            K += (u64)q.length + 1;
        }
        if (K) {
            DevBuf<u64> dn;
            FGPU_TRY(dn.alloc(ctx, (size_t)K));
            FGPU_TRY(b.grow(dwalk, walks.size(), 0));
            FGPU_TRY(ctx->h2d(dwalk.p, walks.data(), walks.size() * sizeof(SpWalk)));
            FGPU_TRY(launch(spb_walk_kernel, dim3(((u32)walks.size() + 63) / 64), dim3(64), 0, st, (const SpWalk*)dwalk.p,
                            (u32)walks.size(), (const u64*)b.word.p, (const u32*)b.par.p, n, dn.p));
            const size_t had = hnodes.size();
            hnodes.resize(had + (size_t)K);
            FGPU_TRY(ctx->d2h(hnodes.data() + had, dn.p, (size_t)K * sizeof(u64)));
        }

        // ---- the claim words this group set, for the next one ----
        if (g + 1 < groups && !segs.empty()) {
            rd.clear();
            for (const spb::Seg& s : segs) {
                SpDesc d = {};
                d.slot = s.slot;
                d.side = s.side;
                d.qbase = s.base;
                d.cnt = s.cnt;
                spb::push_desc(rd, d);
            }
            FGPU_TRY(b.upload(rd.desc));
            FGPU_TRY(launch(spb_reset_kernel, dim3(capped_grid(ctx, rd.rows, 256, 8)), dim3(256), 0, st, (const SpDesc*)b.desc.p,
                            (u32)rd.desc.size(), (u32)rd.rows, (const u32*)b.pool.p, b.word.p, n));
        }
    }
    FGPU_HIP(hipStreamSynchronize(st));
    for (u64 i = 0; i < count; ++i) node_off[i + 1] += node_off[i];
    const u64 P = node_off[count];
    FGPU_REQUIRE(P == hnodes.size(), FGPU_DEVICE, "%s: the groups' paths do not add up", who);
    if (P) {
        ResultBuf out;
        FGPU_REQUIRE(out.alloc(ctx, P * sizeof(u64)), FGPU_OOM, "%s: host allocation failed", who);
        memcpy(out.p, hnodes.data(), P * sizeof(u64));
        *nodes = (uint64_t*)out.release();
    }
    return FGPU_OK;
}
