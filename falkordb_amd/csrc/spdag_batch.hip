// spdag_batch.hip — fgpu_shortest_dag_batch: fgpu_shortest_dag (spdag.hip) for a whole batch of (src, dst) queries, what an
// AllShortestPathsOp fed a parent batch of rows asks for.  The algorithm is the single call's, with a query dimension: the
// single call is bound by its ~25 launches and ~12 counter read-backs, not by its work (profiles/NOTES_r17.md section 6.3), so a
// GROUP of up to `slots` queries advances in lock-step rounds and shares each round's launches and its one read-back.
//
// State of a group.  Every slot has its own dense level words, lvl[(2 * slot + side) * n + v], claimed by atomicCAS as in the
// single call, and its own mark bits for the two sweeps; that is all that is sized by slots x n (8 n + n / 4 bytes per slot).
// Everything else — frontier queues, meeting lists, sweep queues, pairs — lives in two pools the group shares, in segments the
// host reserves before the launch that fills them (spdag_plan.hpp: how long, and why nothing truncates).  The pools grow with
// the entries scanned.
// A round (search or sweep) is: the planner's descriptor table uploaded (SdbDesc: query slot, side, input slice, entry total,
// level, output segments), sdb_lens_kernel writing the row length of every input vertex of every descriptor into one
// concatenated list, one scan_u32 over it, ONE expansion (sweep) launch over the sum of the entry totals, and one read-back of
// the group's counters.  A lane maps its entry to a descriptor by a search over the descriptors' entry prefix, then to an
// input row by csr_row_of inside the descriptor's slice of the scanned list.  A wavefront may straddle descriptors: its
// appends run once per descriptor present in the wave (one iteration almost always), each a ballot compaction with one
// atomicAdd, and the row lengths of the claimed vertices are summed per wave.
// Every query picks its side from its own frontier counts by the single call's rule, keeps the cycle shape's first backward
// expansion, and leaves the table when it has met, died or reached max_hops: lengths, pairs and stats equal the single call's.
// Phase 2 runs the two sweeps of every found query as two descriptors of the same launches.  The pairs of a query, scattered
// over the segments of its sweep rounds, are copied behind one another (sdb_compact_kernel); queries of at most SD_SORT_MAX
// pairs are then ordered by one workgroup each in ONE launch (sd_sort_block) that writes the group's result columns at the
// query's offset; a larger DAG takes the single call's builder path on its own.
// Between groups the level words and mark bits are restored by walking the segments (sdb_reset_kernel): a search claims
// thousands of vertices out of millions, and clearing slots x 8 n bytes per group would cost more than the searches.
//
// The concurrency rules are those of spdag.hip: the level words of a query's expanding side change by atomicCAS only (one side
// per query and launch); its other side, and both in the sweeps, are read-only inside a launch; pool slots are handed out by
// counters, written once with plain stores and read by LATER launches; the mark words change by atomicOr only (the reset
// stores zeros into them in a launch of its own).  Nothing polls or spins.  Nothing is cached on the matrices; the call runs on
// the calling thread's lane.  No kernel spills; static LDS: 32 KiB in the sort, none elsewhere; no dynamic LDS.
#include <vector>

#include "spdag.hpp"
#include "spdag_plan.hpp"

namespace fgpu {

using sdb::SdbCtl;
using sdb::SdbDesc;

// the last descriptor j with key(d[j]) <= x (the keys ascend, key(d[0]) == 0)
__device__ __forceinline__ u32 sdb_by_entry(const SdbDesc* __restrict__ d, u32 nd, u32 x) {
    u32 lo = 0, hi = nd;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (d[mid].ebase <= x) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u32 sdb_by_row(const SdbDesc* __restrict__ d, u32 nd, u32 x) {
    u32 lo = 0, hi = nd;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (d[mid].cbase <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// a lane per query of the group: pool[2 j] = src and pool[2 j + 1] = dst are in place; the levels of the seeds and the counters
__global__ void sdb_seed_kernel(const u32* __restrict__ arp, const u32* __restrict__ atrp, const u32* __restrict__ pool, u32 gn,
                                u32* __restrict__ lvl, u32 n, SdbCtl* __restrict__ ctl) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= gn) return;
    const u32 src = pool[2 * j], dst = pool[2 * j + 1];
    lvl[(size_t)(2 * j) * n + src] = 0;
    if (src != dst) lvl[(size_t)(2 * j + 1) * n + dst] = 0;   // (the cycle shape: dst's backward copy stays unset)
    ctl[2 * j].tail = 1;
    ctl[2 * j].ent = arp[src + 1] - arp[src];
    ctl[2 * j + 1].tail = 1;
    ctl[2 * j + 1].ent = atrp[dst + 1] - atrp[dst];
}

// lcat[i] = the row length of the i-th input vertex of the launch, in the matrix its descriptor reads (a direct descriptor: 1,
// an entry per vertex).  sum != nullptr: the lengths are added into the counters instead (the seeds of the sweeps).
__global__ __launch_bounds__(256) void sdb_lens_kernel(const SdbDesc* __restrict__ desc, u32 nd, u32 rows, const u32* __restrict__ pool,
                                                      const u32* __restrict__ arp, const u32* __restrict__ atrp, int sweep,
                                                      u32* __restrict__ lcat, SdbCtl* sum) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        const u32 j = sdb_by_row(desc, nd, i);
        const u32 v = pool[desc[j].qbase + (i - desc[j].cbase)];
        const u32* rp = ((desc[j].side ^ (u32)sweep) & 1u) ? atrp : arp;   // expansion: side's matrix; sweep 0 reads At, sweep 1 A
        const u32 len = desc[j].direct != SD_NONE ? 1u : rp[v + 1] - rp[v];
        if (sum) atomicAdd((unsigned long long*)&sum[2 * desc[j].slot + desc[j].side].ent, (unsigned long long)len);
        else lcat[i] = len;
    }
}

// the `app` lanes of a wavefront — all of one descriptor — append v behind *counter, which stood at c0 before the launch; every
// lane of the wavefront calls
__device__ __forceinline__ void sdb_append(bool app, u32 v, u32* counter, u32 c0, u32* __restrict__ seg, u32 cap, SdbCtl* c, u32 lane) {
    const u64 mask = __ballot(app);
    if (!mask) return;
    u32 base = 0;
    if (lane == 0) base = atomicAdd(counter, (u32)__builtin_popcountll(mask));
    base = __shfl(base, 0, 64);
    if (app) {
        const u64 at = (u64)(base - c0) + wave_slot(mask, lane);
        if (at < cap) seg[at] = v;
        else c->overflow = 1;
    }
}

// the sum of x over the lanes of the wavefront, in every lane
__device__ __forceinline__ u64 sdb_wave_sum(u64 x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// one level of every live query: a lane per entry e < total of the launch; off[] is the exclusive prefix of the launch's
// concatenated row lengths (off[desc.cbase] == desc.ebase)
__global__ __launch_bounds__(256) void sdb_expand_kernel(CsrView a, CsrView at, const SdbDesc* __restrict__ desc, u32 nd, u32 total,
                                                        const u32* __restrict__ off, u32* pool, u32* lvl, u32 n, SdbCtl* ctl) {
    const u32 lane = lane_id();
    for (u32 e0 = blockIdx.x * 256u; e0 < total; e0 += gridDim.x * 256u) {   // (whole waves stay in the loop: the ballots)
        const u32 e = e0 + threadIdx.x;
        const bool act = e < total;
        bool won = false, met = false;
        u32 v = 0, deg = 0, j = 0;
        if (act) {
            j = sdb_by_entry(desc, nd, e);
            const u32 cbase = desc[j].cbase, side = desc[j].side;
            const u32 i = cbase + csr_row_of(off + cbase, desc[j].cnt, e);
            const CsrView& m = side ? at : a;
            v = m.colidx[m.rowptr[pool[desc[j].qbase + (i - cbase)]] + (e - off[i])];
            u32* mine = lvl + (size_t)(2 * desc[j].slot + side) * n;
            const u32* other = lvl + (size_t)(2 * desc[j].slot + (side ^ 1u)) * n;
            if (mine[v] == SD_NONE) won = atomicCAS(&mine[v], SD_NONE, desc[j].level) == SD_NONE;
            if (won) {
                deg = m.rowptr[v + 1] - m.rowptr[v];
                met = other[v] != SD_NONE;
            }
        }
        for (u64 todo = __ballot(act); todo;) {   // once per descriptor present in the wavefront
            const u32 jl = __shfl(j, __ffsll((unsigned long long)todo) - 1, 64);
            const bool in = act && j == jl;
            todo &= ~__ballot(in);
            SdbCtl* c = ctl + 2 * desc[jl].slot + desc[jl].side;
            sdb_append(in && won, v, &c->tail, desc[jl].tail0, pool + desc[jl].obase, desc[jl].ocap, c, lane);
            sdb_append(in && met, v, &c->aux, desc[jl].aux0, pool + desc[jl].abase, desc[jl].acap, c, lane);
            const u64 ents = sdb_wave_sum(in ? deg : 0u);
            if (lane == 0 && ents) atomicAdd((unsigned long long*)&c->ent, (unsigned long long)ents);
        }
    }
}

// one level of every live sweep: the entries u of the input rows with lvl[u] == desc.level are DAG pairs, u is marked and
// appended once.  A direct descriptor (the last level towards dst) emits (vertex, dst) per input vertex and reads nothing.
__global__ __launch_bounds__(256) void sdb_sweep_kernel(CsrView a, CsrView at, const SdbDesc* __restrict__ desc, u32 nd, u32 total,
                                                       const u32* __restrict__ off, u32* pool, const u32* __restrict__ lvl, u32 n,
                                                       u32* bits, u32 mwords, u32* __restrict__ prow, u32* __restrict__ pcol,
                                                       SdbCtl* ctl) {
    const u32 lane = lane_id();
    for (u32 e0 = blockIdx.x * 256u; e0 < total; e0 += gridDim.x * 256u) {   // (whole waves stay in the loop: the ballots)
        const u32 e = e0 + threadIdx.x;
        const bool act = e < total;
        bool hit = false, fresh = false;
        u32 v = 0, u = 0, deg = 0, j = 0;
        if (act) {
            j = sdb_by_entry(desc, nd, e);
            const u32 cbase = desc[j].cbase, side = desc[j].side;
            const u32 i = cbase + csr_row_of(off + cbase, desc[j].cnt, e);
            v = pool[desc[j].qbase + (i - cbase)];
            if (desc[j].direct != SD_NONE) {
                u = desc[j].direct;
                hit = true;
            } else {
                const CsrView& m = side ? a : at;   // towards src over At, towards dst over A
                u = m.colidx[m.rowptr[v] + (e - off[i])];
                hit = lvl[(size_t)(2 * desc[j].slot + side) * n + u] == desc[j].level;
                if (hit) {
                    const u32 bit = 1u << (u & 31);
                    fresh = !(atomicOr(&bits[(size_t)(2 * desc[j].slot + side) * mwords + (u >> 5)], bit) & bit);
                    if (fresh) deg = m.rowptr[u + 1] - m.rowptr[u];
                }
            }
        }
        for (u64 todo = __ballot(act); todo;) {   // once per descriptor present in the wavefront
            const u32 jl = __shfl(j, __ffsll((unsigned long long)todo) - 1, 64);
            const bool in = act && j == jl;
            todo &= ~__ballot(in);
            const u32 side = desc[jl].side;
            SdbCtl* c = ctl + 2 * desc[jl].slot + side;
            const u64 mask = __ballot(in && hit);
            if (mask) {
                u32 base = 0;
                if (lane == 0) base = atomicAdd(&c->aux, (u32)__builtin_popcountll(mask));
                base = __shfl(base, 0, 64);
                if (in && hit) {
                    const u64 k = (u64)(base - desc[jl].aux0) + wave_slot(mask, lane);
                    if (k < desc[jl].acap) {
                        prow[desc[jl].abase + k] = side ? v : u;   // towards src: (u, v); towards dst: (v, u)
                        pcol[desc[jl].abase + k] = side ? u : v;
                    } else {
                        c->overflow = 1;
                    }
                }
            }
            sdb_append(in && fresh, u, &c->tail, desc[jl].tail0, pool + desc[jl].obase, desc[jl].ocap, c, lane);
            const u64 ents = sdb_wave_sum(in ? deg : 0u);
            if (lane == 0 && ents) atomicAdd((unsigned long long*)&c->ent, (unsigned long long)ents);
        }
    }
}

// the pairs of the group's found queries, segment after segment, behind one another: pair i of the launch comes from its
// descriptor's segment of the pair pool
__global__ __launch_bounds__(256) void sdb_compact_kernel(const SdbDesc* __restrict__ desc, u32 nd, u32 rows, const u32* __restrict__ prow,
                                                         const u32* __restrict__ pcol, u32* __restrict__ crow, u32* __restrict__ ccol) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        const u32 j = sdb_by_row(desc, nd, i);
        const u32 at = desc[j].qbase + (i - desc[j].cbase);
        crow[i] = prow[at];
        ccol[i] = pcol[at];
    }
}

// a workgroup per query of at most SD_SORT_MAX pairs (desc: slot, qbase = its offset in the group's pairs, cnt = its pairs,
// level = L): sorted and written to the group's result columns at that offset
__global__ __launch_bounds__(256) void sdb_sort_kernel(const SdbDesc* __restrict__ desc, const u32* __restrict__ crow,
                                                      const u32* __restrict__ ccol, const u32* __restrict__ lvl, u32 n,
                                                      u64* __restrict__ ofrom, u64* __restrict__ oto, u64* __restrict__ odepth) {
    __shared__ u64 s_key[SD_SORT_MAX];
    const SdbDesc d = desc[blockIdx.x];
    const SdDepth depth{lvl + (size_t)(2 * d.slot) * n, lvl + (size_t)(2 * d.slot + 1) * n, d.level};
    sd_sort_block(s_key, crow + d.qbase, ccol + d.qbase, d.cnt, depth, ofrom + d.qbase, oto + d.qbase, odepth + d.qbase);
}

// what the group's searches and sweeps set goes back to "none" / 0: a lane per vertex of every segment (side 0 / 1: the level
// word of that side, 2 / 3: the word of the mark bits of that sweep)
__global__ __launch_bounds__(256) void sdb_reset_kernel(const SdbDesc* __restrict__ desc, u32 nd, u32 rows, const u32* __restrict__ pool,
                                                       u32* __restrict__ lvl, u32 n, u32* __restrict__ bits, u32 mwords) {
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < rows; i += gridDim.x * 256u) {
        const u32 j = sdb_by_row(desc, nd, i);
        const u32 v = pool[desc[j].qbase + (i - desc[j].cbase)], kind = desc[j].side;
        if (kind < 2) lvl[(size_t)(2 * desc[j].slot + kind) * n + v] = SD_NONE;
        else bits[(size_t)(2 * desc[j].slot + (kind - 2)) * mwords + (v >> 5)] = 0;
    }
}

// the device state of a call and the launches of a round
struct SpdagBatch {
    fgpu_ctx* ctx;
    const fgpu_mat* A;
    const fgpu_mat* At;
    u32 n = 0, mwords = 0, slots = 0;
    DevBuf<u32> lvl, bits, pool, lcat, off, prow, pcol, crow, ccol;
    DevBuf<SdbCtl> ctl;   // [2 * slots] of the search, then [2 * slots] of the sweeps
    DevBuf<SdbDesc> desc;
    std::vector<SdbCtl> h;   // as last read: the 2 * gn counters of the phase

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

    fgpu_info upload(const std::vector<SdbDesc>& d) {
        FGPU_TRY(grow(desc, d.size(), 0));
        return ctx->h2d(desc.p, d.data(), d.size() * sizeof(SdbDesc));
    }

    fgpu_info read(int phase, u32 gn) {
        h.resize(2 * (size_t)gn);
        FGPU_TRY(ctx->d2h(h.data(), ctl.p + (size_t)phase * 2 * slots, 2 * (size_t)gn * sizeof(SdbCtl)));
        return FGPU_OK;
    }

    // the launches of one planned round; pool_kept / pairs_kept: what the pools held before the planner reserved for it
    fgpu_info run(const sdb::Round& rd, bool sweep, u64 pool_kept, u64 pool_used, u64 pairs_kept, u64 pairs_used) {
        hipStream_t st = ctx->stream();
        FGPU_TRY(grow(pool, pool_used, pool_kept));
        if (sweep) {
            FGPU_TRY(grow(prow, pairs_used, pairs_kept));
            FGPU_TRY(grow(pcol, pairs_used, pairs_kept));
        }
        FGPU_TRY(grow(lcat, rd.rows, 0));
        FGPU_TRY(grow(off, rd.rows, 0));
        FGPU_TRY(upload(rd.desc));
        const u32 nd = (u32)rd.desc.size(), rows = (u32)rd.rows, total = (u32)rd.entries;
        FGPU_TRY(launch(sdb_lens_kernel, dim3(capped_grid(ctx, rows, 256, 4)), dim3(256), 0, st, (const SdbDesc*)desc.p, nd, rows,
                        (const u32*)pool.p, (const u32*)A->rowptr, (const u32*)At->rowptr, sweep ? 1 : 0, lcat.p, (SdbCtl*)nullptr));
        FGPU_TRY(scan_u32(ctx, lcat.p, off.p, rows, nullptr));
        if (!sweep)
            FGPU_TRY(launch(sdb_expand_kernel, dim3(capped_grid(ctx, total, 256, 8)), dim3(256), 0, st, view_of(A), view_of(At),
                            (const SdbDesc*)desc.p, nd, total, (const u32*)off.p, pool.p, lvl.p, n, ctl.p));
        else
            FGPU_TRY(launch(sdb_sweep_kernel, dim3(capped_grid(ctx, total, 256, 8)), dim3(256), 0, st, view_of(A), view_of(At),
                            (const SdbDesc*)desc.p, nd, total, (const u32*)off.p, pool.p, (const u32*)lvl.p, n, bits.p, mwords, prow.p,
                            pcol.p, ctl.p + 2 * (size_t)slots));
        return FGPU_OK;
    }
};

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_shortest_dag_batch(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* src,
                                             const uint64_t* dst, uint64_t count, int64_t max_hops, uint32_t slots, int64_t* length,
                                             uint64_t* pair_off, uint64_t** from, uint64_t** to, uint64_t** depth, uint64_t* stats) {
    const char* who = "fgpu_shortest_dag_batch";
    FGPU_REQUIRE(ctx && A && length && pair_off && from && to && depth && (count == 0 || (src && dst)), FGPU_NULL_POINTER,
                 "%s: NULL argument", who);
    FGPU_TRY(check_adjacency(who, A, At));
    FGPU_REQUIRE(slots <= sdb::SLOTS_MAX, FGPU_INVALID, "%s: slots %u exceeds %u", who, slots, sdb::SLOTS_MAX);
    const u32 n = (u32)A->nrows;
    if (n)
        for (u64 i = 0; i < count; ++i)
            FGPU_REQUIRE(src[i] < A->nrows && dst[i] < A->nrows, FGPU_OUT_OF_BOUNDS, "%s: %s of query %llu out of range", who,
                         src[i] < A->nrows ? "dst" : "src", (unsigned long long)i);
    FGPU_REQUIRE(A->nnz < 0xFFFFFFFFull && (!At || At->nnz < 0xFFFFFFFFull), FGPU_INVALID, "%s: too many entries", who);
    *from = *to = *depth = nullptr;
    for (u64 i = 0; i < count; ++i) length[i] = -1;
    for (u64 i = 0; i <= count; ++i) pair_off[i] = 0;
    if (stats) memset(stats, 0, (size_t)count * 8 * sizeof(uint64_t));
    if (count == 0 || n == 0 || max_hops == 0 || A->nnz == 0) return FGPU_OK;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, A));
    if (!At) {   // a missing transpose: built once for the call, released with the guard
        FGPU_TRY(mat_transpose_pattern(ctx, &in.dAt.m, A));
        At = in.dAt.get();
    }
    FGPU_TRY(in.at(ctx, At));
    hipStream_t st = ctx->stream();
    const int sides = ctx->opt.spdag_sides;

    SpdagBatch b;
    b.ctx = ctx;
    b.A = A;
    b.At = At;
    b.n = n;
    b.mwords = (u32)(((size_t)n + 31) / 32);
    b.slots = sdb::derive_slots(count, n, slots);
    const size_t S = b.slots;
    FGPU_TRY(b.lvl.alloc(ctx, S * 2 * n));
    FGPU_TRY(b.bits.alloc(ctx, S * 2 * b.mwords));
    FGPU_TRY(b.ctl.alloc(ctx, 4 * S));
    FGPU_HIP(hipMemsetAsync(b.lvl.p, 0xFF, S * 2 * n * sizeof(u32), st));
    FGPU_HIP(hipMemsetAsync(b.bits.p, 0, S * 2 * b.mwords * sizeof(u32), st));

    std::vector<u64> hcol[3];   // the result columns of the groups done so far
    std::vector<sdb::Query> qs;
    std::vector<sdb::Seg> segs;
    std::vector<u32> seeds;
    sdb::Round rd;
    const u64 groups = sdb::group_count(count, b.slots);
    for (u64 g = 0; g < groups; ++g) {
        u64 first;
        u32 gn;
        sdb::group_range(count, b.slots, g, &first, &gn);
        sdb::Pool pool, pairs;
        segs.clear();
        qs.resize(gn);
        seeds.resize(2 * (size_t)gn);
        for (u32 j = 0; j < gn; ++j) {
            sdb::seed_query(qs[j], j, (u32)src[first + j], (u32)dst[first + j]);
            seeds[2 * j] = qs[j].src;
            seeds[2 * j + 1] = qs[j].dst;
            segs.push_back(sdb::Seg{j, 0, 2 * j, 1});
            segs.push_back(sdb::Seg{j, 1, 2 * j + 1, 1});
        }
        pool.reserve(2 * (u64)gn);
        FGPU_TRY(b.grow(b.pool, pool.used, 0));
        FGPU_TRY(ctx->h2d(b.pool.p, seeds.data(), seeds.size() * sizeof(u32)));
        FGPU_HIP(hipMemsetAsync(b.ctl.p, 0, 4 * S * sizeof(SdbCtl), st));
        FGPU_TRY(launch(sdb_seed_kernel, dim3((gn + 63) / 64), dim3(64), 0, st, (const u32*)A->rowptr, (const u32*)At->rowptr,
                        (const u32*)b.pool.p, gn, b.lvl.p, n, b.ctl.p));
        FGPU_TRY(b.read(0, gn));
        for (u32 j = 0; j < gn; ++j) sdb::seed_degrees(qs[j], b.h[2 * j].ent, b.h[2 * j + 1].ent);

        // ---- phase 1: the searches, a level of every live query per round ----
        for (;;) {
            const u64 kept = pool.used;
            FGPU_REQUIRE(sdb::plan_search(qs, sides, max_hops, n, pool, rd), FGPU_INVALID, "%s: the worklists of a group outgrew 2^32", who);
            if (rd.empty()) break;
            FGPU_TRY(b.run(rd, false, kept, pool.used, 0, 0));
            FGPU_TRY(b.read(0, gn));
            FGPU_REQUIRE(sdb::apply_search(qs, rd, b.h.data(), segs), FGPU_DEVICE, "%s: a worklist outgrew its segment", who);
        }

        // ---- phase 2: the DAGs of the found queries, a level of every live sweep per round ----
        sdb::plan_seeds(qs, rd);
        if (!rd.empty()) {
            FGPU_TRY(b.upload(rd.desc));
            FGPU_TRY(launch(sdb_lens_kernel, dim3(capped_grid(ctx, rd.rows, 256, 4)), dim3(256), 0, st, (const SdbDesc*)b.desc.p,
                            (u32)rd.desc.size(), (u32)rd.rows, (const u32*)b.pool.p, (const u32*)A->rowptr, (const u32*)At->rowptr, 1,
                            (u32*)nullptr, b.ctl.p + 2 * S));
            FGPU_TRY(b.read(1, gn));
            sdb::apply_seeds(qs, rd, b.h.data());
            for (;;) {
                const u64 kept = pool.used, pkept = pairs.used;
                FGPU_REQUIRE(sdb::plan_sweeps(qs, n, pool, pairs, rd), FGPU_INVALID, "%s: the pairs of a group outgrew 2^32", who);
                if (rd.empty()) break;
                FGPU_TRY(b.run(rd, true, kept, pool.used, pkept, pairs.used));
                FGPU_TRY(b.read(1, gn));
                FGPU_REQUIRE(sdb::apply_sweeps(qs, rd, b.h.data(), segs), FGPU_DEVICE, "%s: a worklist outgrew its segment", who);
            }
        }

        // ---- the group's pairs: behind one another, ordered per query, out ----
        rd.clear();
        std::vector<SdbDesc> small, large;   // the found queries of at most SD_SORT_MAX pairs, and the others
        for (sdb::Query& q : qs) {
            sdb::SdbDesc t = {};
            t.slot = q.slot;
            t.qbase = (u32)rd.rows;
            t.level = q.length();
            for (const sdb::Seg& s : q.pairs) {
                SdbDesc d = {};
                d.slot = q.slot;
                d.qbase = s.base;
                d.cnt = s.cnt;
                sdb::push_desc(rd, d);
            }
            t.cnt = (u32)(rd.rows - t.qbase);
            pair_off[first + q.slot + 1] = q.n_pairs();   // (counts for now; the prefix is taken at the end)
            if (stats) sdb::fill_stats(q, stats + 8 * (first + q.slot));
            if (q.state != sdb::FOUND) continue;
            FGPU_REQUIRE(t.cnt > 0 && t.cnt == q.n_pairs(), FGPU_DEVICE, "%s: a path of %u hops left no pair", who, t.level);
            length[first + q.slot] = (int64_t)t.level;
            (t.cnt <= SD_SORT_MAX ? small : large).push_back(t);
        }
        const u64 K = rd.rows;
        if (K) {
            FGPU_REQUIRE(K < 0xFFFFFFFFull, FGPU_INVALID, "%s: too many pairs", who);
            FGPU_TRY(b.grow(b.crow, K, 0));
            FGPU_TRY(b.grow(b.ccol, K, 0));
            FGPU_TRY(b.upload(rd.desc));
            FGPU_TRY(launch(sdb_compact_kernel, dim3(capped_grid(ctx, K, 256, 8)), dim3(256), 0, st, (const SdbDesc*)b.desc.p,
                            (u32)rd.desc.size(), (u32)K, (const u32*)b.prow.p, (const u32*)b.pcol.p, b.crow.p, b.ccol.p));
            DevBuf<u64> trip;
            FGPU_TRY(trip.alloc(ctx, 3 * (size_t)K));
            if (!small.empty()) {
                FGPU_TRY(b.upload(small));
                FGPU_TRY(launch(sdb_sort_kernel, dim3((u32)small.size()), dim3(256), 0, st, (const SdbDesc*)b.desc.p, (const u32*)b.crow.p,
                                (const u32*)b.ccol.p, (const u32*)b.lvl.p, n, trip.p, trip.p + K, trip.p + 2 * K));
            }
            for (const SdbDesc& t : large) {   // rare: the single call's builder path, a query at a time
                MatRef f;
                FGPU_TRY(mat_from_device_coo(ctx, &f.m, n, n, b.crow.p + t.qbase, b.ccol.p + t.qbase, t.cnt));
                FGPU_REQUIRE(f->nnz == t.cnt, FGPU_DEVICE, "%s: the DAG lost pairs in the sort", who);
                const SdDepth dep{b.lvl.p + (size_t)(2 * t.slot) * n, b.lvl.p + (size_t)(2 * t.slot + 1) * n, t.level};
                FGPU_TRY(launch(csr_edge_list_kernel<SdDepth>, dim3(capped_grid(ctx, t.cnt, 256, 4)), dim3(256), 0, st, view_of(f.get()),
                                t.cnt, dep, trip.p + t.qbase, trip.p + K + t.qbase, trip.p + 2 * K + t.qbase));
                FGPU_HIP(hipStreamSynchronize(st));   // (f is released at the end of the iteration)
            }
            for (int c = 0; c < 3; ++c) {
                const size_t had = hcol[c].size();
                hcol[c].resize(had + (size_t)K);
                FGPU_TRY(ctx->d2h(hcol[c].data() + had, trip.p + (size_t)c * K, (size_t)K * sizeof(u64)));
            }
        }

        // ---- the level words and mark bits this group set, for the next one ----
        if (g + 1 < groups) {
            rd.clear();
            for (const sdb::Seg& s : segs) {
                SdbDesc d = {};
                d.slot = s.slot;
                d.side = s.kind;
                d.qbase = s.base;
                d.cnt = s.cnt;
                sdb::push_desc(rd, d);
            }
            FGPU_TRY(b.upload(rd.desc));
            FGPU_TRY(launch(sdb_reset_kernel, dim3(capped_grid(ctx, rd.rows, 256, 8)), dim3(256), 0, st, (const SdbDesc*)b.desc.p,
                            (u32)rd.desc.size(), (u32)rd.rows, (const u32*)b.pool.p, b.lvl.p, n, b.bits.p, b.mwords));
        }
    }
    FGPU_HIP(hipStreamSynchronize(st));
    for (u64 i = 0; i < count; ++i) pair_off[i + 1] += pair_off[i];
    const u64 P = pair_off[count];
    FGPU_REQUIRE(P == hcol[0].size(), FGPU_DEVICE, "%s: the groups' pairs do not add up", who);
    if (P) {
        ResultBuf out[3];
        for (int c = 0; c < 3; ++c) {
            FGPU_REQUIRE(out[c].alloc(ctx, P * sizeof(u64)), FGPU_OOM, "%s: host allocation failed", who);
            memcpy(out[c].p, hcol[c].data(), P * sizeof(u64));
        }
        *from = (uint64_t*)out[0].release();
        *to = (uint64_t*)out[1].release();
        *depth = (uint64_t*)out[2].release();
    }
    return FGPU_OK;
}
