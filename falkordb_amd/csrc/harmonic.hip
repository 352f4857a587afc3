// harmonic.hip — algo.HarmonicCentrality's numeric core: LAGr_HarmonicCentrality (called from graph/src/runtime/functions/
// algo_procedures.rs:2623-2784) over the boolean directed adjacency A.  HyperBall: every vertex carries a HyperLogLog sketch of
// its out-ball, 1024 one-byte registers; C_0[v] holds v's own (slot, rank); C_t[v] = the bytewise max of C_{t-1}[v] and of
// C_{t-1}[w] over the stored entries (v, w) of row v; a vertex whose sketch changed adds (count(C_t[v]) - est_{t-1}[v]) / t to
// its score; the run ends after the first iteration that changes no sketch (the rules are restated in include/fgpu.h).
//
// The hot loop is a gather of whole 1 KiB rows.  One wavefront owns one destination row and holds it as one uint4 per lane;
// a neighbour's sketch arrives as one coalesced 1 KiB load (lane l reads bytes 16 l .. 16 l + 15), HC_INFLIGHT of them in
// flight per wave; the merge is a per-byte unsigned max on packed dwords (registers are <= 23, so the carry-free SWAR compare
// of hc_max_u8x4 applies).  The estimate is fused behind the last neighbour: the wave compares the merged row with the old
// one (ballot), reduces sum 2^(23 - r) and the zero count across the lanes, and lane 0 writes the estimate and the score.
//
// What an iteration reads (all of it bit-identical to merging every entry, because registers only grow):
//   - chg_{t-1}[w], a byte per vertex: did w's sketch change in iteration t - 1 (all ones before the first).  C_{t-1}[v]
//     already holds max C_{t-2}[w], so only the entries whose column changed are gathered;
//   - a row with no such entry whose own sketch did not change either is skipped: the buffer it would be written to still
//     holds C_{t-2}[v] = C_{t-1}[v].  A row that changed itself is carried over into the other buffer.
// Hub rows (>= HUB_DEG entries, the snapshot's hub_chunks triples) take two launches: hc_hub_partial_kernel gives a workgroup
// per chunk, a quarter of the chunk per wave, the four partial sketches folded through 4 KiB of LDS into partial[chunk];
// hc_hub_fold_kernel gives a wave per hub row, which folds the row's old sketch and its chunks' partial sketches and runs the
// same fused estimate.  Max is idempotent: no atomics.
//
// Concurrency rules (per-XCD L2s are not coherent inside a launch; MI355X_MICROARCH.md):
//   - inside a launch C_{t-1}, chg_{t-1} and partial[] are only read, and every byte of C_t, chg_t, est and score is written by
//     the one wave that owns the row; partial[] is written by the launch before the one that reads it;
//   - all ordering between the two row classes and between the iterations is by kernel boundaries on the context's stream.
//     Nothing polls or spins;
//   - every iteration kernel adds its changed sketches into cnt[j] (block_add_u64) and returns at once when cnt[j - 1] == 0,
//     i.e. when the previous iteration changed nothing: the host launches HC_BATCH iterations per read-back.  After an
//     iteration that changed nothing both buffers hold the same sketches, so the parity of the skipped launches is harmless.
// Static LDS: 4 KiB (hub partial); no dynamic LDS.
#include <math.h>

#include "algo.hpp"

namespace fgpu {

constexpr u32 HC_M = 1024;        // registers per sketch, one byte each
constexpr u32 HC_Q = HC_M / 16;   // uint4 per sketch = lanes per wavefront
constexpr u32 HC_BATCH = 4;       // iterations launched per read-back of the changed counters
constexpr u32 HC_INFLIGHT = 4;    // neighbour rows a wave has in flight
static_assert(HC_Q == WAVE, "a wavefront holds one sketch, 16 registers per lane");
constexpr double HC_ALPHA_MM = 0.7213 / (1.0 + 1.079 / 1024.0) * 1024.0 * 1024.0;

// the murmur3 32-bit finaliser of the row index: slot = the top 10 bits, rank = 1 + the leading zeros of the low 22 bits
// written in 22 bits, 23 when they are all zero (vertex 0: slot 0, rank 23)
__device__ __forceinline__ void hc_hash(u32 v, u32& slot, u32& rank) {
    u32 h = v;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    slot = h >> 22;
    const u32 w = h & 0x3FFFFFu;
    rank = w ? (u32)__clz((int)w) - 9u : 23u;
}

// the estimate of a sketch from sum23 = sum over its registers of 2^(23 - r) (an integer <= 2^33: S is exact) and its zeros
__device__ __forceinline__ double hc_count(u64 sum23, u32 zeros) {
    const double S = (double)sum23 * (1.0 / 8388608.0);
    double E = HC_ALPHA_MM / S;
    if (E <= 2560.0 && zeros > 0u) E = 1024.0 * log(1024.0 / (double)zeros);
    else if (E > 4294967296.0 / 30.0) E = -4294967296.0 * log(1.0 - E / 4294967296.0);
    return E;
}

// per-byte unsigned max of two packed dwords whose bytes are all < 128 (registers are <= 23): with bit 7 of every byte of a
// set, a - b borrows across no byte boundary and leaves bit 7 set exactly where a's byte >= b's
__device__ __forceinline__ u32 hc_max_u8x4(u32 a, u32 b) {
    const u32 m = ((((a | 0x80808080u) - b) >> 7) & 0x01010101u) * 0xFFu;
    return (a & m) | (b & ~m);
}
__device__ __forceinline__ uint4 hc_max(uint4 a, uint4 b) {
    return make_uint4(hc_max_u8x4(a.x, b.x), hc_max_u8x4(a.y, b.y), hc_max_u8x4(a.z, b.z), hc_max_u8x4(a.w, b.w));
}

__device__ __forceinline__ void hc_sum_word(u32 x, u32& s, u32& z) {
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 r = (x >> (8 * k)) & 0xFFu;
        s += 1u << (23u - r);
        z += r == 0u ? 1u : 0u;
    }
}

// the estimate of the sketch a wave holds (acc: 16 registers per lane), the same value in every lane
__device__ __forceinline__ double hc_wave_count(uint4 acc) {
    u32 s = 0, z = 0;   // per lane s <= 16 x 2^23
    hc_sum_word(acc.x, s, z); hc_sum_word(acc.y, s, z); hc_sum_word(acc.z, s, z); hc_sum_word(acc.w, s, z);
    u64 sum = s;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        z += __shfl_xor(z, d, 64);
    }
    return hc_count(sum, z);
}

// folds into acc the sketches of the lanes of `mask`, whose vertex is in that lane's w: HC_INFLIGHT rows in flight
__device__ __forceinline__ uint4 hc_gather(uint4 acc, const uint4* __restrict__ in, u32 w, u64 mask, u32 lane) {
    while (mask) {
        uint4 r[HC_INFLIGHT];
#pragma unroll
        for (u32 k = 0; k < HC_INFLIGHT; ++k) {
            r[k] = make_uint4(0u, 0u, 0u, 0u);
            if (mask) {   // (wave-uniform)
                const u32 src = (u32)__builtin_ctzll(mask);
                mask &= mask - 1ull;
                const u32 x = __builtin_amdgcn_readfirstlane(__shfl(w, (int)src, 64));
                r[k] = in[(size_t)x * HC_Q + lane];
            }
        }
#pragma unroll
        for (u32 k = 0; k < HC_INFLIGHT; ++k) acc = hc_max(acc, r[k]);
    }
    return acc;
}

// the merged row acc of vertex v against its old row: writes C_t[v], and est / score when the sketch changed (returned)
__device__ __forceinline__ bool hc_finish_row(uint4 acc, uint4 old, uint4* __restrict__ out, double* __restrict__ est,
                                              double* __restrict__ score, u32 v, u32 t, u32 lane) {
    out[(size_t)v * HC_Q + lane] = acc;
    if (!__ballot(acc.x != old.x || acc.y != old.y || acc.z != old.z || acc.w != old.w)) return false;
    const double E = hc_wave_count(acc);
    if (lane == 0) {
        score[v] += (E - est[v]) / (double)t;
        est[v] = E;
    }
    return true;
}

// C_0 into buffer 0 (both buffers zeroed before), est_0, and chg_0 = "active"
__global__ __launch_bounds__(256) void hc_init_kernel(const u64* __restrict__ act, u32 n, uint8_t* __restrict__ c0,
                                                     double* __restrict__ est, uint8_t* __restrict__ chg0) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const bool on = vertex_on(act, v);
        chg0[v] = on ? 1 : 0;
        if (!on) { est[v] = 0.0; continue; }
        u32 slot, rank;
        hc_hash(v, slot, rank);
        c0[(size_t)v * HC_M + slot] = (uint8_t)rank;
        est[v] = hc_count((u64)(HC_M - 1) * 8388608ull + (1ull << (23u - rank)), HC_M - 1);
    }
}

// iteration t over the rows of fewer than HUB_DEG entries, a wavefront per row.  work[0] += entries of the recomputed rows,
// work[1] += sketches gathered
__global__ __launch_bounds__(256) void hc_rows_kernel(CsrView a, const u64* __restrict__ act, const uint4* __restrict__ in,
                                                     uint4* __restrict__ out, const uint8_t* __restrict__ cprev,
                                                     uint8_t* __restrict__ ccur, double* __restrict__ est,
                                                     double* __restrict__ score, u32 n, u32 t, const unsigned long long* prev,
                                                     unsigned long long* cnt, unsigned long long* work) {
    if (prev && *prev == 0ull) return;
    const u32 lane = lane_id();
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6;
    const u64 nwaves = ((u64)gridDim.x * 256) >> 6;
    u64 changed = 0, entries = 0, gathered = 0;   // (lane 0 counts)
    for (u64 vv = wave; vv < n; vv += nwaves) {
        const u32 v = (u32)vv;
        const u32 b = a.rowptr[v], deg = a.rowptr[v + 1] - b;
        if (deg >= HUB_DEG) continue;   // the hub kernels' row
        bool have = vertex_on(act, v) && cprev[v] != 0;   // an inactive row never changes, nor does it change anyone
        uint4 old = make_uint4(0u, 0u, 0u, 0u), acc = old;
        if (have) { old = in[(size_t)v * HC_Q + lane]; acc = old; }
        u32 ng = 0;
        if (vertex_on(act, v)) {
            for (u32 c = 0; c < deg; c += 64) {
                const bool mine = c + lane < deg;
                const u32 w = mine ? a.colidx[b + c + lane] : 0u;
                const u64 mask = __ballot(mine && cprev[w] != 0);
                if (!mask) continue;
                if (!have) { old = in[(size_t)v * HC_Q + lane]; acc = old; have = true; }
                ng += (u32)__builtin_popcountll(mask);
                acc = hc_gather(acc, in, w, mask, lane);
            }
        }
        bool moved = false;
        if (have) moved = hc_finish_row(acc, old, out, est, score, v, t, lane);
        if (lane == 0) {
            ccur[v] = moved ? 1 : 0;
            changed += moved ? 1u : 0u;
            entries += have ? deg : 0u;
            gathered += ng;
        }
    }
    block_add_u64(changed, cnt);
    block_add_u64(entries, &work[0]);
    block_add_u64(gathered, &work[1]);
}

// ---- hub rows -------------------------------------------------------------------------------------------------------------
// Chunk h = (row, cb, ce) of the snapshot's list; the chunks of a row are consecutive in it and cb = rowptr[row] + k HUB_CHUNK
// (hub_scan_kernel).  partial[h] = the max over the chunk's entries whose column changed (zero when there is none).
__global__ __launch_bounds__(256) void hc_hub_partial_kernel(const u32* __restrict__ chunks, u32 n_chunks,
                                                            const u32* __restrict__ colidx, const u64* __restrict__ act,
                                                            const uint4* __restrict__ in, const uint8_t* __restrict__ cprev,
                                                            uint4* __restrict__ partial, const unsigned long long* prev,
                                                            unsigned long long* work) {
    if (prev && *prev == 0ull) return;
    __shared__ uint4 s[4 * HC_Q];
    const u32 lane = lane_id(), wv = threadIdx.x >> 6;
    u64 gathered = 0;
    for (u32 h = blockIdx.x; h < n_chunks; h += gridDim.x) {
        const u32 row = chunks[3 * h], cb = chunks[3 * h + 1], ce = chunks[3 * h + 2];
        if (!vertex_on(act, row)) continue;   // (workgroup-uniform)
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
        for (u32 c = cb + wv * 64; c < ce; c += 256) {
            const bool mine = c + lane < ce;
            const u32 w = mine ? colidx[c + lane] : 0u;
            const u64 mask = __ballot(mine && cprev[w] != 0);
            if (!mask) continue;
            if (lane == 0) gathered += (u32)__builtin_popcountll(mask);
            acc = hc_gather(acc, in, w, mask, lane);
        }
        s[wv * HC_Q + lane] = acc;
        __syncthreads();
        if (wv == 0)
            partial[(size_t)h * HC_Q + lane] = hc_max(hc_max(acc, s[HC_Q + lane]), hc_max(s[2 * HC_Q + lane], s[3 * HC_Q + lane]));
        __syncthreads();   // s is reused by the next chunk
    }
    block_add_u64(gathered, &work[1]);
}

// a wave per hub row (its first chunk speaks for it): the old sketch, the chunks' partial sketches, the fused estimate
__global__ __launch_bounds__(256) void hc_hub_fold_kernel(const u32* __restrict__ chunks, u32 n_chunks, const u32* __restrict__ rowptr,
                                                         const u64* __restrict__ act, const uint4* __restrict__ in,
                                                         uint4* __restrict__ out, const uint4* __restrict__ partial,
                                                         uint8_t* __restrict__ ccur, double* __restrict__ est,
                                                         double* __restrict__ score, u32 t, const unsigned long long* prev,
                                                         unsigned long long* cnt, unsigned long long* work) {
    if (prev && *prev == 0ull) return;
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    u64 changed = 0, entries = 0;
    for (u32 h = wave; h < n_chunks; h += nwaves) {
        const u32 row = chunks[3 * h];
        const u32 rs = rowptr[row], deg = rowptr[row + 1] - rs;
        if (chunks[3 * h + 1] != rs) continue;
        bool moved = false;
        if (vertex_on(act, row)) {
            const uint4 old = in[(size_t)row * HC_Q + lane];
            uint4 acc = old;
            const u32 nk = (deg + HUB_CHUNK - 1) / HUB_CHUNK;
            for (u32 k = 0; k < nk; ++k) acc = hc_max(acc, partial[(size_t)(h + k) * HC_Q + lane]);
            moved = hc_finish_row(acc, old, out, est, score, row, t, lane);
            if (lane == 0) entries += deg;
        }
        if (lane == 0) {
            ccur[row] = moved ? 1 : 0;
            changed += moved ? 1u : 0u;
        }
    }
    block_add_u64(changed, cnt);
    block_add_u64(entries, &work[0]);
}

// reachable[v] = llround(est[v]) - 1 (-1 outside the bitmap); tot[0] = the largest, tot[1] = vertices with a non-zero score
__global__ __launch_bounds__(256) void hc_finish_kernel(const double* __restrict__ est, const double* __restrict__ score,
                                                       const u64* __restrict__ act, u32 n, long long* __restrict__ reach,
                                                       unsigned long long* tot) {
    u64 top = 0, nz = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        long long r = -1;
        if (vertex_on(act, v)) {
            r = llround(est[v]) - 1;
            if (r > 0 && (u64)r > top) top = (u64)r;
            nz += score[v] != 0.0 ? 1u : 0u;
        }
        reach[v] = r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(top, d, 64);
        top = o > top ? o : top;
    }
    if (lane_id() == 0 && top) atomicMax(&tot[0], (unsigned long long)top);
    block_add_u64(nz, &tot[1]);
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_harmonic(fgpu_ctx* ctx, const fgpu_mat* A, const uint64_t* active_bitmap, double* score,
                                   int64_t* reachable, uint8_t* registers, uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && A && score && reachable, FGPU_NULL_POINTER, "fgpu_harmonic: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_harmonic", A, nullptr));
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)A->nrows;
    if (n == 0) return FGPU_OK;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, A));
    FGPU_TRY(mat_ensure_finalized(A));   // the hub list
    hipStream_t st = ctx->stream();
    DevBuf<u64> act;
    DevBuf<uint8_t> regs, chg;
    DevBuf<uint4> partial;
    DevBuf<double> fp;
    DevBuf<long long> reach;
    DevBuf<unsigned long long> cnt;
    if (active_bitmap) FGPU_TRY(upload_active(ctx, act, active_bitmap, n));
    const u64* a = act.p;
    const CsrView av = view_of(A);
    const size_t row_bytes = (size_t)n * HC_M;
    const u32 nch = A->n_hub_chunks;
    FGPU_TRY(regs.alloc(ctx, 2 * row_bytes));   // C_{t-1} and C_t
    FGPU_TRY(chg.alloc(ctx, 2 * (size_t)n));
    FGPU_TRY(fp.alloc(ctx, 2 * (size_t)n));     // est, score
    FGPU_TRY(reach.alloc(ctx, n));
    FGPU_TRY(cnt.alloc(ctx, HC_BATCH + 4));     // changed per launched iteration; entries, gathered; largest reachable, non-zero scores
    if (nch) FGPU_TRY(partial.alloc(ctx, (size_t)nch * HC_Q));
    double* est = fp.p;
    double* sc = fp.p + n;
    unsigned long long* work = cnt.p + HC_BATCH;
    FGPU_HIP(hipMemsetAsync(regs.p, 0, 2 * row_bytes, st));
    FGPU_HIP(hipMemsetAsync(sc, 0, (size_t)n * sizeof(double), st));
    FGPU_HIP(hipMemsetAsync(work, 0, 4 * sizeof(unsigned long long), st));
    const u32 vgrid = capped_grid(ctx, n, 256, 8);
    FGPU_TRY(launch(hc_init_kernel, dim3(vgrid), dim3(256), 0, st, a, n, regs.p, est, chg.p));
    uint8_t* buf[2] = {regs.p, regs.p + row_bytes};
    uint8_t* flag[2] = {chg.p, chg.p + n};
    const u32 rgrid = capped_grid(ctx, n, 4, 8);   // a wave per row
    const u32 hgrid = hub_grid(ctx, A);
    u64 iters = 0, changes = 0;
    u32 cur = 0, t = 0;   // buf[cur] and flag[cur] hold C_t and "changed in iteration t"
    bool done = false;
    while (!done) {
        FGPU_HIP(hipMemsetAsync(cnt.p, 0, HC_BATCH * sizeof(unsigned long long), st));
        for (u32 j = 0; j < HC_BATCH; ++j) {
            const unsigned long long* prev = j ? cnt.p + j - 1 : nullptr;
            unsigned long long* c = cnt.p + j;
            const uint4* src = (const uint4*)buf[cur];
            uint4* dst = (uint4*)buf[cur ^ 1];
            FGPU_TRY(launch(hc_rows_kernel, dim3(rgrid), dim3(256), 0, st, av, a, src, dst, (const uint8_t*)flag[cur],
                            flag[cur ^ 1], est, sc, n, t + j + 1, prev, c, work));
            if (nch) {
                FGPU_TRY(launch(hc_hub_partial_kernel, dim3(hgrid), dim3(256), 0, st, (const u32*)A->hub_chunks.p, nch, av.colidx,
                                a, src, (const uint8_t*)flag[cur], partial.p, prev, work));
                FGPU_TRY(launch(hc_hub_fold_kernel, dim3(capped_grid(ctx, nch, 4, 8)), dim3(256), 0, st,
                                (const u32*)A->hub_chunks.p, nch, av.rowptr, a, src, dst, (const uint4*)partial.p, flag[cur ^ 1],
                                est, sc, t + j + 1, prev, c, work));
            }
            cur ^= 1;
        }
        u32 w[2 * HC_BATCH];
        FGPU_TRY(read_words(ctx, (const u32*)cnt.p, 2 * HC_BATCH, w));   // one read-back per batch
        for (u32 j = 0; j < HC_BATCH && !done; ++j) {
            const u64 moved = (u64)w[2 * j] | ((u64)w[2 * j + 1] << 32);
            ++t;
            if (moved == 0) done = true;   // the launches behind it returned at once: both buffers hold these sketches
            else { ++iters; changes += moved; }
        }
    }
    FGPU_TRY(launch(hc_finish_kernel, dim3(vgrid), dim3(256), 0, st, (const double*)est, (const double*)sc, a, n, reach.p,
                    work + 2));
    FGPU_TRY(ctx->d2h(score, sc, (size_t)n * sizeof(double)));   // one DMA each when the arrays are pinned
    FGPU_TRY(ctx->d2h(reachable, reach.p, (size_t)n * sizeof(int64_t)));
    if (registers) FGPU_TRY(ctx->d2h(registers, buf[cur], row_bytes));
    unsigned long long tot[4];
    FGPU_TRY(ctx->d2h(tot, work, sizeof(tot)));
    ctx->hc_last_entries.store(tot[0], std::memory_order_relaxed);
    ctx->hc_last_gathered.store(tot[1], std::memory_order_relaxed);
    if (stats) {
        stats[0] = iters;
        stats[1] = changes;
        stats[2] = tot[2];
        stats[3] = tot[3];
    }
    FGPU_HIP(hipStreamSynchronize(st));
    return FGPU_OK;
}
