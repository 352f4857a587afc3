// exists.hip — the last hop of a pattern predicate (fgpu_expand_exists): one bit per source row, "does the row reach anything".
//
// The last hop's rule is the row-level mask of Matrix::delta_lmxm, R_i = ((F·m)<not (F·dm)> U (F·dp)) & label, so a destination
// a row reaches through m can still be masked by ANOTHER frontier vertex of the same row.  Existence is decided per vertex
// where it can be and per row only where it must:
//   D      the columns that occur in dm (one bitmap; absent when dm is empty);
//   P[u]   the dp row of u has a label-passing entry, or the m row of u has a label-passing entry outside D: no tombstone
//          masks that destination for any row, so every row whose frontier holds u matches ("sure");
//   Q[u]   the m row of u has a label-passing entry inside D ("maybe").
// Rows with maybe and not sure go to the caller's exact pass.  A vertex' row is walked with an early exit at the first P;
// without a label and without D, P[u] is "the m or dp row is not empty" and no entry is read at all.
//
// Two forms.  exists_csr_kernel: a wavefront per source row walks its frontier 64 vertices at a time — a lane evaluates a
// short vertex row by itself, the wavefront takes the long ones together 64 entries a step — and stops at the first sure
// vertex: the work is the frontier plus the entries scanned, never a pass over the vertices.  The bit state:
// exists_pq_kernel evaluates P and Q of every flagged vertex (exists_long_rows_kernel the long rows, a wavefront each), then
// exists_bits_kernel ORs the state rows of the P (Q) vertices into a per-workgroup accumulator in LDS, a tile of EX_TILE words
// at a time, and pushes each workgroup's non-zero words into the result with one atomicOr per word.
#include "common.hpp"

namespace fgpu {

constexpr u32 EX_LONG = 64;      // rows of more entries (m + dp) are walked by a wavefront, 64 entries a step
constexpr u32 EX_TILE = 512;     // words per accumulator and tile of the bit form: 2 x 4 KiB of LDS
constexpr u32 EX_VERTS = 4096;   // vertices per workgroup and tile of exists_bits_kernel

struct ExLayers {
    CsrView m, dp;       // dp.rowptr == nullptr: no dp layer
    const u64* label;    // nullable, one bit per column
    const u64* dcols;    // nullable, D
};

__device__ __forceinline__ bool ex_bit(const u64* __restrict__ b, u32 v) { return (b[v >> 6] >> (v & 63)) & 1ull; }

__device__ __forceinline__ void ex_ranges(const ExLayers& L, u32 u, u32& mb, u32& me, u32& pb, u32& pe) {
    row_range(L.m, u, mb, me);
    if (L.dp.rowptr) row_range(L.dp, u, pb, pe);
    else { pb = 0; pe = 0; }
}

// one lane, one vertex: bit 0 = P, bit 1 = Q (Q is not looked for once P holds)
__device__ __forceinline__ u32 ex_eval_lane(const ExLayers& L, u32 mb, u32 me, u32 pb, u32 pe, u32& read) {
    if (!L.label && !L.dcols) return (me > mb || pe > pb) ? 1u : 0u;
    if (pe > pb) {
        if (!L.label) return 1u;
        for (u32 q = pb; q < pe; ++q) {
            ++read;
            if (ex_bit(L.label, L.dp.colidx[q])) return 1u;
        }
    }
    u32 r = 0;
    for (u32 q = mb; q < me; ++q) {
        ++read;
        const u32 v = L.m.colidx[q];
        if (L.label && !ex_bit(L.label, v)) continue;
        if (L.dcols && ex_bit(L.dcols, v)) r |= 2u;
        else return r | 1u;
    }
    return r;
}

// the whole wavefront, one vertex (the ranges are wave-uniform): 64 entries a step, stopping at the step that finds P
__device__ __forceinline__ u32 ex_eval_wave(const ExLayers& L, u32 mb, u32 me, u32 pb, u32 pe, u32 lane, u32& read) {
    if (!L.label && !L.dcols) return (me > mb || pe > pb) ? 1u : 0u;
    if (pe > pb) {
        if (!L.label) return 1u;
        for (u32 q0 = pb; q0 < pe; q0 += 64) {
            const u32 q = q0 + lane;
            bool p = false;
            if (q < pe) { ++read; p = ex_bit(L.label, L.dp.colidx[q]); }
            if (__ballot(p) != 0ull) return 1u;
        }
    }
    u32 r = 0;
    for (u32 q0 = mb; q0 < me; q0 += 64) {
        const u32 q = q0 + lane;
        bool p = false, d = false;
        if (q < me) {
            ++read;
            const u32 v = L.m.colidx[q];
            if (!L.label || ex_bit(L.label, v)) {
                d = L.dcols && ex_bit(L.dcols, v);
                p = !d;
            }
        }
        if (__ballot(p) != 0ull) return r | 1u;
        if (__ballot(d) != 0ull) r |= 2u;
    }
    return r;
}

__device__ __forceinline__ void ex_add_read(unsigned long long* entries, u32 read) {
    for (int o = 32; o > 0; o >>= 1) read += __shfl_xor(read, o);
    if (lane_id() == 0 && read) atomicAdd(entries, (unsigned long long)read);
}

// D: a bit per column that occurs in dm
__global__ __launch_bounds__(256) void exists_dm_cols_kernel(const u32* __restrict__ col, u32 nnz, u64* __restrict__ dcols) {
    for (u32 q = blockIdx.x * 256 + threadIdx.x; q < nnz; q += gridDim.x * 256) {
        const u32 v = col[q];
        atomicOr((unsigned long long*)&dcols[v >> 6], 1ull << (v & 63));
    }
}

// ---- the CSR frontier: a wavefront per source row ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void exists_csr_kernel(CsrView f, ExLayers L, u32 k, u64* __restrict__ sure, u64* __restrict__ maybe,
                                                         unsigned long long* __restrict__ entries) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    u32 read = 0;
    for (u32 i = wave; i < k; i += nwaves) {
        u32 fb, fe;
        row_range(f, i, fb, fe);
        bool is_sure = false, is_maybe = false;
        for (u32 q0 = fb; q0 < fe && !is_sure; q0 += 64) {
            const u32 q = q0 + lane;
            u32 r = 0, mb = 0, me = 0, pb = 0, pe = 0;
            bool longv = false;
            if (q < fe) {
                ex_ranges(L, f.colidx[q], mb, me, pb, pe);
                longv = (L.label || L.dcols) && (me - mb) + (pe - pb) > EX_LONG;
                if (!longv) r = ex_eval_lane(L, mb, me, pb, pe, read);
            }
            if (__ballot(r & 1u) != 0ull) { is_sure = true; break; }
            if (__ballot(r & 2u) != 0ull) is_maybe = true;
            unsigned long long todo = __ballot(longv);
            while (todo) {
                const int l = __ffsll(todo) - 1;
                todo &= todo - 1;
                const u32 rr = ex_eval_wave(L, __shfl(mb, l), __shfl(me, l), __shfl(pb, l), __shfl(pe, l), lane, read);
                if (rr & 1u) { is_sure = true; break; }
                if (rr & 2u) is_maybe = true;
            }
        }
        if (lane == 0) {
            if (is_sure) atomicOr((unsigned long long*)&sure[i >> 6], 1ull << (i & 63));
            else if (is_maybe) atomicOr((unsigned long long*)&maybe[i >> 6], 1ull << (i & 63));
        }
    }
    ex_add_read(entries, read);
}

// ---- the bit state -------------------------------------------------------------------------------------------------------------
// pq[v] = P | Q << 1 for every vertex (0 where the state's row is not flagged); a long row gets 0x80 and is listed for
// exists_long_rows_kernel
__global__ __launch_bounds__(256) void exists_pq_kernel(ExLayers L, u32 n, const uint8_t* __restrict__ flag, uint8_t* __restrict__ pq,
                                                        u32* __restrict__ long_list, u32* __restrict__ n_long,
                                                        unsigned long long* __restrict__ entries) {
    u32 read = 0;
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) {
        u32 r = 0;
        if (!flag || flag[v]) {
            u32 mb, me, pb, pe;
            ex_ranges(L, v, mb, me, pb, pe);
            if ((L.label || L.dcols) && (me - mb) + (pe - pb) > EX_LONG) {
                long_list[atomicAdd(n_long, 1u)] = v;
                r = 0x80u;
            } else {
                r = ex_eval_lane(L, mb, me, pb, pe, read);
            }
        }
        pq[v] = (uint8_t)r;
    }
    // (every lane of the wavefront is back here: the loop's exits differ by one trip at most)
    ex_add_read(entries, read);
}

__global__ __launch_bounds__(256) void exists_long_rows_kernel(ExLayers L, const u32* __restrict__ long_list, const u32* __restrict__ n_long,
                                                               uint8_t* __restrict__ pq, unsigned long long* __restrict__ entries) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 nl = *n_long;
    u32 read = 0;
    for (u32 j = wave; j < nl; j += nwaves) {
        const u32 v = long_list[j];
        u32 mb, me, pb, pe;
        ex_ranges(L, v, mb, me, pb, pe);
        const u32 r = ex_eval_wave(L, mb, me, pb, pe, lane, read);
        if (lane == 0) pq[v] = (uint8_t)r;
    }
    ex_add_read(entries, read);
}

// workgroup (bx, by): vertices [bx * EX_VERTS, ...), words [by * EX_TILE, ...) of every state row.  A wavefront lists its 64
// vertices' hits in LDS, then reads `per` = 64 / span of their rows a step, a lane per word.
__global__ __launch_bounds__(256) void exists_bits_kernel(const u64* __restrict__ x, u32 ws, u32 w, u32 n, const uint8_t* __restrict__ pq,
                                                          bool want_maybe, u64* __restrict__ sure,
                                                          u64* __restrict__ maybe) {
    __shared__ u64 acc[2][EX_TILE];
    __shared__ u32 hits[4][64];
    const u32 lane = lane_id(), wv = threadIdx.x >> 6;
    const u32 w0 = blockIdx.y * EX_TILE;
    const u32 tw = (w - w0) < EX_TILE ? (w - w0) : EX_TILE;      // words of this tile
    for (u32 j = threadIdx.x; j < tw; j += 256) { acc[0][j] = 0ull; acc[1][j] = 0ull; }
    __syncthreads();
    u32 span = 1;                                               // lanes per vertex: the tile's words rounded up to a power of two, <= 64
    while (span < tw && span < 64) span <<= 1;
    const u32 per = 64 / span, sub = lane / span, jl = lane % span;
    const u32 v_begin = blockIdx.x * EX_VERTS;
    const u32 v_end = (n - v_begin) < EX_VERTS ? n : v_begin + EX_VERTS;
    for (u32 v0 = v_begin + wv * 64; v0 < v_end; v0 += 256) {
        const u32 v = v0 + lane;
        u32 r = 0;
        if (v < v_end) r = pq[v] & (want_maybe ? 3u : 1u);
        const unsigned long long hm = __ballot(r != 0);
        if (!hm) continue;
        if (r) hits[wv][__popcll(hm & ((1ull << lane) - 1ull))] = v | (r << 30);   // (n < 2^30: see exists_rows)
        const u32 nh = (u32)__popcll(hm);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the list is read by other lanes of this wavefront
        __builtin_amdgcn_wave_barrier();
        for (u32 h0 = 0; h0 < nh; h0 += per) {
            const u32 h = h0 + sub;
            if (h >= nh) continue;
            const u32 e = hits[wv][h], u = e & 0x3FFFFFFFu, rr = e >> 30;
            const u64* row = x + (size_t)u * ws + w0;
            for (u32 j = jl; j < tw; j += span) {
                const u64 word = row[j];
                if (!word) continue;
                // P rows are sure; a vertex with Q alone adds to maybe
                u64* a = &acc[(rr & 1u) ? 0 : 1][j];
                if (word & ~*(volatile u64*)a) atomicOr((unsigned long long*)a, (unsigned long long)word);
            }
        }
        __builtin_amdgcn_wave_barrier();                        // (the next trip's list goes into the same slots)
    }
    __syncthreads();
    for (u32 j = threadIdx.x; j < tw; j += 256) {
        if (acc[0][j]) atomicOr((unsigned long long*)&sure[w0 + j], (unsigned long long)acc[0][j]);
        if (acc[1][j]) atomicOr((unsigned long long*)&maybe[w0 + j], (unsigned long long)acc[1][j]);
    }
}

fgpu_info exists_rows(fgpu_ctx* ctx, const fgpu_mat* f, const BitState* s, const fgpu_mat* m, const fgpu_mat* dp, const fgpu_mat* dm,
                      const u64* label_dev, u32 k, u64* sure, u64* maybe, u32 words, u64* entries) {
    if (k == 0) return FGPU_OK;
    hipStream_t st = ctx->stream();
    const bool has_dp = dp && dp->nnz, has_dm = dm && dm->nnz;
    if (!m->nnz && !has_dp) return FGPU_OK;                       // nothing to reach
    ExLayers L;
    L.m = view_of(m);
    if (has_dp) L.dp = view_of(dp);
    else { L.dp.rowptr = nullptr; L.dp.colidx = nullptr; L.dp.hrows = nullptr; L.dp.nvec = 0; L.dp.nrows = 0; }
    L.label = label_dev;
    L.dcols = nullptr;
    DevBuf<u64> dcols;
    if (has_dm) {
        const u64 nw = (m->ncols + 63) / 64;
        FGPU_TRY(dcols.alloc(ctx, nw + 1));
        FGPU_HIP(hipMemsetAsync(dcols.p, 0, (nw + 1) * sizeof(u64), st));
        ProfScope ps(ctx, "exists_dm_cols_kernel", dm->nnz * 4);
        u32 grid = cdiv(dm->nnz, 256);
        if (grid > (u32)ctx->cus * 8) grid = ctx->cus * 8;
        FGPU_TRY(launch(exists_dm_cols_kernel, dim3(grid), dim3(256), 0, st, (const u32*)dm->colidx, (u32)dm->nnz, dcols.p));
        L.dcols = dcols.p;
    }
    DevBuf<unsigned long long> cnt;
    FGPU_TRY(cnt.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), st));
    if (f) {
        if (f->nnz) {
            ProfScope ps(ctx, "exists_csr_kernel", (u64)k * 8 + f->nnz * 12);
            u32 grid = cdiv(k, 4);
            if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
            FGPU_TRY(launch(exists_csr_kernel, dim3(grid), dim3(256), 0, st, view_of(f), L, k, sure, maybe, cnt.p));
        }
    } else {
        FGPU_REQUIRE(s && s->x.p && (!s->lazy || s->flag.p) && !s->perm, FGPU_INVALID, "fgpu_expand_exists: bad bit state");
        FGPU_REQUIRE(m->nrows == s->n, FGPU_DIM_MISMATCH, "fgpu_expand_exists: matrix has %llu rows, frontier %u",
                     (unsigned long long)m->nrows, s->n);
        FGPU_REQUIRE(s->n < (1u << 30), FGPU_INVALID, "fgpu_expand_exists: the bit form takes fewer than 2^30 vertices");
        FGPU_REQUIRE(words >= s->w, FGPU_INVALID, "fgpu_expand_exists: result narrower than the state");
        const u32 n = s->n;
        DevBuf<uint8_t> pq;
        DevBuf<u32> long_list, n_long;
        FGPU_TRY(pq.alloc(ctx, (size_t)n + 1));
        FGPU_TRY(long_list.alloc(ctx, (size_t)n + 1));
        FGPU_TRY(n_long.alloc(ctx, 1));
        FGPU_HIP(hipMemsetAsync(n_long.p, 0, sizeof(u32), st));
        u32 grid = cdiv(n, 256);
        if (grid > (u32)ctx->cus * 8) grid = ctx->cus * 8;
        {
            ProfScope ps(ctx, "exists_pq_kernel", (u64)n * 10);
            FGPU_TRY(launch(exists_pq_kernel, dim3(grid), dim3(256), 0, st, L, n, (const uint8_t*)s->flag.p, pq.p, long_list.p, n_long.p,
                            cnt.p));
        }
        if (L.label || L.dcols) {
            ProfScope ps(ctx, "exists_long_rows_kernel", 0);
            FGPU_TRY(launch(exists_long_rows_kernel, dim3(ctx->cus * 4), dim3(256), 0, st, L, (const u32*)long_list.p, (const u32*)n_long.p,
                            pq.p, cnt.p));
        }
        {
            ProfScope ps(ctx, "exists_bits_kernel", (u64)n + s->nz_rows * s->w * 8);
            FGPU_TRY(launch(exists_bits_kernel, dim3(cdiv(n, EX_VERTS), cdiv(s->w, EX_TILE)), dim3(256), 0, st, (const u64*)s->x.p, s->ws,
                            s->w, n, (const uint8_t*)pq.p, has_dm, sure, maybe));
        }
    }
    u64 got = 0;
    FGPU_TRY(read_u64(ctx, (const u64*)cnt.p, &got));
    if (entries) *entries += got;
    return FGPU_OK;
}

}  // namespace fgpu
