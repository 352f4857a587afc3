// wcc.hip — algo.WCC's numeric core: LAGr_ConnectedComponents (called from graph/src/runtime/functions/algo_procedures.rs:789-880
// through lagraph_bindings.rs:521-526) over the undirected view of an adjacency matrix.  component[v] = the smallest vertex id
// of v's component — the labelling LAGraph's FastSV converges to (its hooking only ever lowers a parent), which makes the
// output deterministic whatever order the hooks below race in.
//
// Afforest (Sutton, Ben-Nun, Barak 2018), the union-find GAP and ECL-CC-class GPU codes use, over a parent forest parent[n]:
//   1. parent[v] = v
//   2. WCC_ROUNDS neighbour rounds: round r links every active vertex to the r-th entry of its row of A (skipped when that
//      neighbour is inactive), a compress follows each round
//   3. a fixed-seed sample of WCC_SAMPLES vertices picks the most frequent root c (the giant component, on R-MAT)
//   4. every vertex whose root is not c links the rest of its row of A (entries r >= WCC_ROUNDS) and all of its row of At;
//      then a final compress, and one pass that counts the roots and widens the labels to int64 on the device.
// Phase 4 is what makes this pay: the edges of the giant component are never read again.  It is correct only because BOTH
// directions of every edge are walked: an edge (u, w) is skipped only when u and w were each seen inside c's tree, i.e. when
// they are connected already.  Without At the caller promises a symmetric pattern (LAGraph's is_symmetric_structure), and A's
// rows hold both directions.  wcc_mode 2 (and small graphs under auto) is one link pass over every entry of A: each stored
// entry joins its two endpoints, so At is not needed there.
//
// The parent forest, its hooks and its compression are the prelude's (algo.hpp, "the union-find forest", with the concurrency
// rules): every link below is a forest_hook, and kernel boundaries separate the link, compress, sample and count phases.
// No dynamic LDS; the static LDS of the word kernel is 2 KiB per workgroup, the sample kernel's 4 KiB.
#include "algo.hpp"

namespace fgpu {

constexpr u32 WCC_ROUNDS = 2;          // Afforest's neighbour rounds
constexpr u32 WCC_SAMPLES = 1024;      // vertices sampled for the giant component (one workgroup)
constexpr u64 WCC_SEED = 0x57CC2018ull;
constexpr u32 WCC_NONE = 0xFFFFFFFFu;
constexpr u32 WCC_AUTO_MIN_N = 4096;   // wcc_mode 0: Afforest from this many vertices, the full pass below

// phase 2: round r links v to the r-th entry of its row
__global__ __launch_bounds__(256) void wcc_link_round_kernel(CsrView a, const u64* __restrict__ act, u32* parent, u32 n, u32 r,
                                                            unsigned long long* entries) {
    u64 took = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        if (!vertex_on(act, v)) continue;
        const u32 b = a.rowptr[v], e = a.rowptr[v + 1];
        if (e - b <= r) continue;
        const u32 w = a.colidx[b + r];
        ++took;
        if (vertex_on(act, w)) forest_hook(parent, v, w);
    }
    block_add_u64(took, entries);
}

// phases 4 and the full pass, rows shorter than HUB_DEG: entries [first, deg) of every row whose vertex is active and not in
// the giant's tree (giant == nullptr: every row).  A wavefront per 64-row word, entry-parallel over the word's contiguous entry
// range (the row of an entry by a 6-step search of the word's offsets in LDS, as pr_spmv_kernel): a row of any length below
// HUB_DEG costs its entries, not a lane's serial walk.
__global__ __launch_bounds__(256) void wcc_link_words_kernel(CsrView a, const u64* __restrict__ act, u32* parent, u32 n, u32 first,
                                                            const u32* giant, unsigned long long* entries) {
    __shared__ u32 s_off[4][65];   // exclusive prefix of the word's effective row lengths
    __shared__ u32 s_rb[4][64];    // first entry to read of each row
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    const u32 nwords = (n + 63) >> 6;
    const u32 c = giant ? *giant : WCC_NONE;
    const u32* __restrict__ col = a.colidx;
    u32* off = s_off[wv];
    u32* rbs = s_rb[wv];
    u64 seen = 0;
    for (u32 g = wave; g < nwords; g += nwaves) {
        const u32 v = (g << 6) + lane;
        u32 rb = 0, re = 0;
        if (v < n) { rb = a.rowptr[v]; re = a.rowptr[v + 1]; }
        const bool take = v < n && re - rb > first && re - rb < HUB_DEG && vertex_on(act, v) && (c == WCC_NONE || parent[v] != c);
        const u32 len = take ? re - rb - first : 0u;
        u32 inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = __shfl_up(inc, d, 64);
            if (lane >= (u32)d) inc += y;
        }
        off[lane + 1] = inc;
        if (lane == 0) off[0] = 0;
        rbs[lane] = rb + first;
        const u32 total = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        if (lane == 0) seen += total;
        for (u32 e0 = 0; e0 < total; e0 += 64) {
            const u32 e = e0 + lane;
            if (e >= total) continue;
            u32 lo = 0, hi = 64;   // largest lo with off[lo] <= e
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const u32 mid = (lo + hi) >> 1;
                if (off[mid] <= e) lo = mid; else hi = mid;
            }
            const u32 w = col[rbs[lo] + (e - off[lo])];
            if (vertex_on(act, w)) forest_hook(parent, (g << 6) + lo, w);
        }
    }
    block_add_u64(seen, entries);
}

// the same for the rows of HUB_DEG entries and more: a workgroup per chunk of the snapshot's static hub list (mat_finalize)
__global__ __launch_bounds__(256) void wcc_link_hubs_kernel(const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ rowptr,
                                                           const u32* __restrict__ col, const u64* __restrict__ act, u32* parent,
                                                           u32 first, const u32* giant, unsigned long long* entries) {
    __shared__ u32 s_take;
    const u32 c = giant ? *giant : WCC_NONE;
    u64 seen = 0;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 row = hub[3 * h], e = hub[3 * h + 2];
        u32 b = hub[3 * h + 1];
        const u32 lo = rowptr[row] + first;
        if (b < lo) b = lo;
        // one decision for the whole workgroup (the threads' plain loads of parent[row] need not agree)
        if (threadIdx.x == 0) s_take = (b < e && vertex_on(act, row) && (c == WCC_NONE || parent[row] != c)) ? 1u : 0u;
        __syncthreads();
        const bool take = s_take != 0;
        __syncthreads();
        if (!take) continue;
        if (threadIdx.x == 0) seen += e - b;
        for (u32 i = b + threadIdx.x; i < e; i += 256) {
            const u32 w = col[i];
            if (vertex_on(act, w)) forest_hook(parent, row, w);
        }
    }
    if (threadIdx.x == 0 && seen) atomicAdd(entries, (unsigned long long)seen);
}

// phase 3: the most frequent root among WCC_SAMPLES fixed-seed samples (ties: the smaller root); inactive samples do not vote.
// One workgroup: the roots sorted in LDS (bitonic), the longest run wins.
__global__ __launch_bounds__(WCC_SAMPLES) void wcc_sample_kernel(const u32* __restrict__ parent, const u64* __restrict__ act, u32 n,
                                                                u32* __restrict__ giant) {
    __shared__ u32 s[WCC_SAMPLES];
    __shared__ unsigned long long best;
    const u32 t = threadIdx.x;
    const u32 v = (u32)(mix64(WCC_SEED + t) % n);
    s[t] = vertex_on(act, v) ? parent[v] : WCC_NONE;
    if (t == 0) best = 0ull;
    __syncthreads();
    for (u32 k = 2; k <= WCC_SAMPLES; k <<= 1) {
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            const u32 p = t ^ j;
            if (p > t) {
                const u32 x = s[t], y = s[p];
                if ((x > y) == ((t & k) == 0)) { s[t] = y; s[p] = x; }
            }
            __syncthreads();
        }
    }
    const u32 x = s[t];
    if (x != WCC_NONE && (t == 0 || s[t - 1] != x)) {
        u32 e = t + 1;
        while (e < WCC_SAMPLES && s[e] == x) ++e;
        atomicMax(&best, ((unsigned long long)(e - t) << 32) | (unsigned long long)(WCC_NONE - x));
    }
    __syncthreads();
    if (t == 0) *giant = best ? WCC_NONE - (u32)(best & 0xFFFFFFFFull) : WCC_NONE;
}

// the flat forest -> int64 labels (-1 for inactive vertices); cnt[0] += roots among the active vertices, cnt[1] += the size of
// the tree the sampled giant ended in
__global__ __launch_bounds__(256) void wcc_finish_kernel(const u32* __restrict__ parent, const u64* __restrict__ act, u32 n,
                                                        const u32* __restrict__ giant, long long* __restrict__ out,
                                                        unsigned long long* cnt) {
    const u32 c = giant ? *giant : WCC_NONE;
    const u32 gc = c != WCC_NONE ? parent[c] : WCC_NONE;
    u64 roots = 0, gsz = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        if (!vertex_on(act, v)) { out[v] = -1; continue; }
        const u32 r = parent[v];
        out[v] = (long long)r;
        roots += r == v ? 1u : 0u;
        gsz += r == gc ? 1u : 0u;
    }
    block_add_u64(roots, &cnt[0]);
    block_add_u64(gsz, &cnt[1]);
}

// entries [first, deg) of every row of M (giant: skip the rows of that tree; nullptr = none): the word pass + the hub chunks
static fgpu_info wcc_link_rows(fgpu_ctx* ctx, const fgpu_mat* m, const u64* act, u32* parent, u32 n, u32 first, const u32* giant,
                               unsigned long long* entries, u64* launches) {
    const u32 nwords = cdiv(n, 64);
    u32 grid = cdiv(nwords, 4);
    if (grid > (u32)ctx->cus * 8) grid = (u32)ctx->cus * 8;
    FGPU_TRY(launch(wcc_link_words_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(m), act, parent, n, first, giant,
                    entries));
    ++*launches;
    if (m->n_hub_chunks) {
        FGPU_TRY(launch(wcc_link_hubs_kernel, dim3(hub_grid(ctx, m)), dim3(256), 0, ctx->stream(), (const u32*)m->hub_chunks.p,
                        m->n_hub_chunks, (const u32*)m->rowptr, (const u32*)m->colidx, act, parent, first, giant, entries));
        ++*launches;
    }
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_wcc(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                              int64_t* component, uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && A && component, FGPU_NULL_POINTER, "fgpu_wcc: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_wcc", A, At));
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)A->nrows;
    if (n == 0) return FGPU_OK;
    const int mode = ctx->opt.wcc_mode ? ctx->opt.wcc_mode : (n >= WCC_AUTO_MIN_N ? 1 : 2);
    const bool afforest = mode == 1;
    // a NULL At is the caller's promise of a symmetric pattern; the full pass reads every entry of A once, each joins both of
    // its endpoints, and never needs At
    if (!afforest) At = nullptr;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, A));
    FGPU_TRY(in.at(ctx, At));
    FGPU_TRY(mat_ensure_finalized(A));   // the hub lists
    if (At) FGPU_TRY(mat_ensure_finalized(At));
    DevBuf<u64> act;
    DevBuf<u32> parent, giant, flags;
    DevBuf<unsigned long long> cnt;
    DevBuf<long long> wide;
    if (active_bitmap) FGPU_TRY(upload_active(ctx, act, active_bitmap, n));
    FGPU_TRY(parent.alloc(ctx, n));
    FGPU_TRY(giant.alloc(ctx, 1));
    FGPU_TRY(flags.alloc(ctx, FOREST_MAX_JUMPS));
    FGPU_TRY(cnt.alloc(ctx, 3));   // entries read, roots, giant size
    FGPU_TRY(wide.alloc(ctx, n));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, 3 * sizeof(unsigned long long), ctx->stream()));
    FGPU_HIP(hipMemsetAsync(giant.p, 0xFF, sizeof(u32), ctx->stream()));
    const u64* a = act.p;
    const u32 grid = capped_grid(ctx, n, 256, 4);   // keeps the count atomics few
    FGPU_TRY(forest_init(ctx, parent.p, n));
    u64 launches = 0;
    if (afforest) {
        for (u32 r = 0; r < WCC_ROUNDS; ++r) {
            FGPU_TRY(launch(wcc_link_round_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(A), a, parent.p, n, r,
                            cnt.p));
            ++launches;
            FGPU_TRY(forest_compress(ctx, "fgpu_wcc", parent.p, n, flags.p));
        }
        FGPU_TRY(launch(wcc_sample_kernel, dim3(1), dim3(WCC_SAMPLES), 0, ctx->stream(), (const u32*)parent.p, a, n, giant.p));
        FGPU_TRY(wcc_link_rows(ctx, A, a, parent.p, n, WCC_ROUNDS, giant.p, cnt.p, &launches));
        if (At) FGPU_TRY(wcc_link_rows(ctx, At, a, parent.p, n, 0, giant.p, cnt.p, &launches));
    } else {
        FGPU_TRY(wcc_link_rows(ctx, A, a, parent.p, n, 0, nullptr, cnt.p, &launches));
    }
    FGPU_TRY(forest_compress(ctx, "fgpu_wcc", parent.p, n, flags.p));
    FGPU_TRY(launch(wcc_finish_kernel, dim3(grid), dim3(256), 0, ctx->stream(), (const u32*)parent.p, a, n,
                    afforest ? (const u32*)giant.p : nullptr, wide.p, cnt.p + 1));
    FGPU_TRY(ctx->d2h(component, wide.p, (size_t)n * sizeof(int64_t)));   // one DMA when component[] is pinned
    if (stats) {
        unsigned long long h[3];
        FGPU_TRY(ctx->d2h(h, cnt.p, sizeof(h)));
        stats[0] = h[1];
        stats[1] = h[0];
        stats[2] = launches;
        stats[3] = afforest ? h[2] : 0;
    }
    FGPU_HIP(hipStreamSynchronize(ctx->stream()));
    return FGPU_OK;
}
