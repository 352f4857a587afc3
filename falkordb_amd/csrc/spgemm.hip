// spgemm.hip — ANY_PAIR (structural) sparse products and the CondTraverse expansion core.
//
// Reference call sites (graph/src/graph/graphblas/matrix.rs unless noted):
//   Matrix::lmxm        :930-947   C = F x B, GrB_mxm(GxB_ANY_PAIR_BOOL), no mask
//   Matrix::delta_lmxm  :1317-1402 (F x (m U dp)) with (F x dm) masked out of the F x m part
//   expand_batch        runtime/ops/cond_traverse.rs:452-751 (F build :600-601, chain :602-605,
//                       ascending (row, dest) read-out :644, dst label post-filter :647-651)
//
// The semiring never reads values, so a product row is the sorted union of the B-rows named
// by the F-row.  Device formulation: (1) per F-entry degree + prefix sum = output upper bound
// ("flops"), (2) one wavefront per F-entry copies its B-row coalesced into the row's segment,
// (3) segments with more than one source go through segsort_unique (prims.hip), single-source
// segments (hop 1 of every traversal) are already sorted and unique, (4) compaction to CSR.
#include <algorithm>
#include <string>
#include <thread>

#include "common.hpp"

namespace fgpu {

__global__ void entry_deg_kernel(CsrView f, CsrView b, u32 nnzf, u32* __restrict__ deg) {
    u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnzf) { if (e == nnzf) deg[e] = 0; return; }
    u32 s = f.colidx[e], rb, re;
    row_range(b, s, rb, re);
    deg[e] = re - rb;
}

__global__ void gather_u64_kernel(const u64* __restrict__ eoff, const u32* __restrict__ frp, u32 k,
                                  u64* __restrict__ roff, u32* __restrict__ maxlen) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > k) return;
    roff[i] = eoff[frp[i]];
    if (i < k) {
        u32 len = frp[i + 1] - frp[i];
        u32 m = len;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { u32 o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        if (lane_id() == 0 && m > 1) atomicMax(maxlen, m);
        else if (lane_id() == 0 && m == 1) atomicMax(maxlen, 1u);
    }
}

// one wavefront per F entry: copy the B row it names into the product row's segment
__global__ __launch_bounds__(256) void gather_rows_kernel(CsrView f, CsrView b, u32 nnzf,
                                                         const u64* __restrict__ eoff, u32* __restrict__ tmp) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    for (u32 e = wave; e < nnzf; e += nwaves) {
        u32 s = f.colidx[e], rb, re;
        row_range(b, s, rb, re);
        const u64 o = eoff[e];
        u32 i = rb + lane;
        // 4 x 64 per trip keeps several loads in flight for long rows
        for (; i + 192 < re; i += 256) {
            u32 x0 = b.colidx[i], x1 = b.colidx[i + 64], x2 = b.colidx[i + 128], x3 = b.colidx[i + 192];
            u64 p = o + (i - rb);
            tmp[p] = x0; tmp[p + 64] = x1; tmp[p + 128] = x2; tmp[p + 192] = x3;
        }
        for (; i < re; i += 64) tmp[o + (i - rb)] = b.colidx[i];
    }
}

__global__ void seg_len_kernel(const u64* __restrict__ roff, u32 k, u32* __restrict__ cnt) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > k) return;
    cnt[i] = (i < k) ? (u32)(roff[i + 1] - roff[i]) : 0u;
}

// keep entries whose column bit is set in `bitmap`
__global__ __launch_bounds__(256) void bitmap_filter_fill_kernel(CsrView c, const u64* __restrict__ bitmap,
                                                                u32 nrows, u32* __restrict__ tmp,
                                                                u32* __restrict__ cnt) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    const u32* __restrict__ b32 = (const u32*)bitmap;
    for (u32 r = wave; r < nrows; r += nwaves) {
        const u32 rb = c.rowptr[r], re = c.rowptr[r + 1];
        u32 outn = 0;
        for (u32 i0 = rb; i0 < re; i0 += 64) {
            u32 i = i0 + lane, x = 0;
            bool keep = false;
            if (i < re) {
                x = c.colidx[i];
                keep = (b32[x >> 5] >> (x & 31)) & 1u;
            }
            u64 mask = __ballot(keep);
            if (keep) tmp[rb + outn + __popcll(mask & ((1ull << lane) - 1ull))] = x;
            outn += (u32)__popcll(mask);
        }
        if (lane == 0) cnt[r] = outn;
    }
}

__global__ __launch_bounds__(256) void compact_rows_kernel(const u32* __restrict__ tmp, const u32* __restrict__ srcoff,
                                                          const u32* __restrict__ rowptr, u32 nrows,
                                                          u32* __restrict__ col) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    for (u32 r = wave; r < nrows; r += nwaves) {
        u32 s = srcoff[r], o = rowptr[r], c = rowptr[r + 1] - o;
        for (u32 i = lane; i < c; i += 64) col[o + i] = tmp[s + i];
    }
}

// (rowmap, nullable: row r of c stands for row rowmap[r] of the call — a pass of a whole-frontier call; rowhash, nullable:
// row r's hash itself — a pass whose rows stand for classes of call rows, expand_count_scan below)
__global__ __launch_bounds__(256) void checksum_kernel(CsrView c, u32 nrows, unsigned long long* __restrict__ acc,
                                                       const u32* __restrict__ rowmap, const u64* __restrict__ rowhash) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    u64 sum = 0;
    for (u32 r = wave; r < nrows; r += nwaves) {
        const u32 rb = c.rowptr[r], re = c.rowptr[r + 1];
        const u64 hr = rowhash ? rowhash[r] : cs_row_hash(rowmap ? rowmap[r] : r);
        for (u32 i = rb + lane; i < re; i += 64) sum += hr * cs_dest_hash(c.colidx[i]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0 && sum) atomicAdd(acc, (unsigned long long)sum);
}

// sum_{(i,s) in F} deg_B(s): the entries a sorted-CSR product would gather (exact, one small pass)
static fgpu_info mxm_flops(fgpu_ctx* ctx, const fgpu_mat* F, const fgpu_mat* B, u64* T) {
    *T = 0;
    const u32 nnzf = (u32)F->nnz;
    if (nnzf == 0 || B->nnz == 0) return FGPU_OK;
    DevBuf<u32> deg;
    DevBuf<u64> eoff, tot;
    FGPU_TRY(deg.alloc(ctx, (size_t)nnzf + 1));
    FGPU_TRY(eoff.alloc(ctx, (size_t)nnzf + 1));
    FGPU_TRY(tot.alloc(ctx, 1));
    FGPU_TRY(launch(entry_deg_kernel, dim3(cdiv((u64)nnzf + 1, 256)), dim3(256), 0, ctx->stream(), view_of(F),
                    view_of(B), nnzf, deg.p));
    FGPU_TRY(scan_u32_to_u64(ctx, deg.p, eoff.p, (u64)nnzf + 1, tot.p));
    return read_u64(ctx, tot.p, T);
}

// entry-parallel form for results with few, very long rows (dense k-hop results: ~10^6 entries per row):
// each lane takes one entry and finds its row in the short row-pointer array
__global__ __launch_bounds__(256) void checksum_entries_kernel(CsrView c, u32 nrows, u32 nnz,
                                                              unsigned long long* __restrict__ acc, const u32* __restrict__ rowmap,
                                                              const u64* __restrict__ rowhash) {
    u64 sum = 0;
    for (u32 q = blockIdx.x * 256 + threadIdx.x; q < nnz; q += gridDim.x * 256) {
        u32 lo = 0, hi = nrows - 1;
        while (lo < hi) {
            u32 mid = (lo + hi + 1) >> 1;
            if (c.rowptr[mid] <= q) lo = mid; else hi = mid - 1;
        }
        sum += (rowhash ? rowhash[lo] : cs_row_hash(rowmap ? rowmap[lo] : lo)) * cs_dest_hash(c.colidx[q]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane_id() == 0 && sum) atomicAdd(acc, (unsigned long long)sum);
}

static fgpu_info empty_dense(fgpu_ctx* ctx, fgpu_mat** out, u64 nrows, u64 ncols) {
    MatRef o;
    FGPU_TRY(mat_alloc(ctx, &o.m, nrows, ncols, 0, false, 0, false));
    const hipError_t e = hipMemsetAsync(o->rowptr, 0, (nrows + 1) * sizeof(u32), ctx->stream());
    FGPU_REQUIRE(e == hipSuccess, FGPU_DEVICE, "memset failed: %s", hipGetErrorString(e));
    *out = o.release();
    return FGPU_OK;
}

// C = F x B (structural).  *flops (nullable) += sum_{(i,s) in F} deg_B(s).
fgpu_info mxm_device(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* F, const fgpu_mat* B, u64* flops) {
    FGPU_REQUIRE(F->ncols == B->nrows, FGPU_DIM_MISMATCH, "mxm: F is %llu x %llu but B is %llu x %llu",
                 (unsigned long long)F->nrows, (unsigned long long)F->ncols, (unsigned long long)B->nrows,
                 (unsigned long long)B->ncols);
    const u64 k = F->nrows;
    const u32 nnzf = (u32)F->nnz;
    if (nnzf == 0 || B->nnz == 0) return empty_dense(ctx, out, k, B->ncols);
    DevBuf<u32> frp, deg, cnt, rowptr, maxlen;
    DevBuf<u64> eoff, roff, tot;
    FGPU_TRY(dense_rowptr(ctx, F, frp));
    FGPU_TRY(deg.alloc(ctx, (size_t)nnzf + 1));
    FGPU_TRY(eoff.alloc(ctx, (size_t)nnzf + 1));
    FGPU_TRY(tot.alloc(ctx, 1));
    FGPU_TRY(launch(entry_deg_kernel, dim3(cdiv((u64)nnzf + 1, 256)), dim3(256), 0, ctx->stream(), view_of(F),
                    view_of(B), nnzf, deg.p));
    FGPU_TRY(scan_u32_to_u64(ctx, deg.p, eoff.p, (u64)nnzf + 1, tot.p));
    FGPU_TRY(roff.alloc(ctx, k + 1));
    FGPU_TRY(maxlen.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(maxlen.p, 0, sizeof(u32), ctx->stream()));
    FGPU_TRY(launch(gather_u64_kernel, dim3(cdiv(k + 1, 256)), dim3(256), 0, ctx->stream(), (const u64*)eoff.p,
                    (const u32*)frp.p, (u32)k, roff.p, maxlen.p));
    u64 T = 0;
    FGPU_TRY(read_u64(ctx, tot.p, &T));
    u32 ml = 0;
    FGPU_TRY(read_u32(ctx, maxlen.p, &ml));
    if (flops) *flops += T;
    if (T == 0) return empty_dense(ctx, out, k, B->ncols);
    FGPU_REQUIRE(T < (1ull << 33), FGPU_OOM,
                 "mxm: %llu gathered entries exceed the per-call workspace; batch the source rows",
                 (unsigned long long)T);
    DevBuf<u32> tmp;
    FGPU_TRY(tmp.alloc(ctx, T));
    {
        ProfScope ps(ctx, "gather_rows_kernel", 12 * (u64)nnzf + 8 * T);   // F entry + B row-pointer pair, B row read + written
        u32 grid = cdiv(nnzf, 4);
        if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
        FGPU_TRY(launch(gather_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(F), view_of(B), nnzf,
                        (const u64*)eoff.p, tmp.p));
    }
    FGPU_TRY(cnt.alloc(ctx, k + 1));
    if (ml <= 1) {
        FGPU_TRY(launch(seg_len_kernel, dim3(cdiv(k + 1, 256)), dim3(256), 0, ctx->stream(), (const u64*)roff.p,
                        (u32)k, cnt.p));
    } else {
        FGPU_HIP(hipMemsetAsync(cnt.p, 0, (k + 1) * sizeof(u32), ctx->stream()));
        ProfScope ps(ctx, "segsort_unique (product rows)", 8 * T);
        FGPU_TRY(segsort_unique(ctx, tmp.p, roff.p, (u32)k, (u32)B->ncols, cnt.p, nullptr));
    }
    FGPU_TRY(rowptr.alloc(ctx, k + 1));
    FGPU_TRY(scan_u32(ctx, cnt.p, rowptr.p, k + 1, nullptr));
    u32 nnz = 0;
    FGPU_TRY(read_u32(ctx, rowptr.p + k, &nnz));
    MatRef o;
    FGPU_TRY(mat_alloc(ctx, &o.m, k, B->ncols, nnz, false, 0, false));
    FGPU_HIP(hipMemcpyAsync(o->rowptr, rowptr.p, (k + 1) * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream()));
    {
        ProfScope ps(ctx, "compact_segments_kernel", 8 * (u64)nnz);
        FGPU_TRY(compact_segments(ctx, tmp.p, roff.p, o->rowptr, (u32)k, o->colidx));
    }
    // hub lists are only needed by BFS; products skip mat_finalize (no extra sync per hop)
    *out = o.release();
    return FGPU_OK;
}

fgpu_info delta_lmxm_device(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* F, const fgpu_mat* m, const fgpu_mat* dp,
                            const fgpu_mat* dm, u64* flops) {
    const bool has_dp = dp && dp->nnz, has_dm = dm && dm->nnz;
    if (!has_dp && !has_dm) return mxm_device(ctx, out, F, m, flops);  // hot path, matrix.rs:1333-1337
    MatRef c, acc, mask;
    if (has_dm) {
        FGPU_TRY(mxm_device(ctx, &mask.m, F, dm, nullptr));
        if (mask->nnz == 0) mask.reset();
    }
    if (has_dp) {
        FGPU_TRY(mxm_device(ctx, &acc.m, F, dp, flops));
        if (acc->nnz == 0) acc.reset();
    }
    FGPU_TRY(mxm_device(ctx, &c.m, F, m, flops));
    if (mask.get() || acc.get()) {
        MatRef merged;
        // (F.m with MASK removed) U ACCUM — the accumulated dp product is not masked (matrix.rs:1382-1400)
        FGPU_TRY(mat_merge_entries(ctx, &merged.m, c.get(), acc.get(), mask.get(), false, c->nrows, c->ncols, true));
        c = std::move(merged);
    }
    mask.reset();
    acc.reset();
    *out = c.release();
    return FGPU_OK;
}

static fgpu_info filter_by_bitmap(fgpu_ctx* ctx, fgpu_mat** out, const fgpu_mat* c, const u64* bitmap_dev) {
    const u64 nrows = c->nrows;
    DevBuf<u32> tmp, cnt, rowptr;
    FGPU_TRY(tmp.alloc(ctx, c->nnz));
    FGPU_TRY(cnt.alloc(ctx, nrows + 1));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, (nrows + 1) * sizeof(u32), ctx->stream()));
    u32 grid = cdiv(nrows ? nrows : 1, 4);
    if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
    if (nrows && c->nnz) {
        FGPU_TRY(launch(bitmap_filter_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(c), bitmap_dev,
                        (u32)nrows, tmp.p, cnt.p));
    }
    FGPU_TRY(rowptr.alloc(ctx, nrows + 1));
    FGPU_TRY(scan_u32(ctx, cnt.p, rowptr.p, nrows + 1, nullptr));
    u32 nnz = 0;
    FGPU_TRY(read_u32(ctx, rowptr.p + nrows, &nnz));
    MatRef o;
    FGPU_TRY(mat_alloc(ctx, &o.m, nrows, c->ncols, nnz, false, 0, false));
    FGPU_HIP(hipMemcpyAsync(o->rowptr, rowptr.p, (nrows + 1) * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream()));
    if (nnz) {
        FGPU_TRY(launch(compact_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream(), (const u32*)tmp.p,
                        (const u32*)c->rowptr, (const u32*)o->rowptr, (u32)nrows, o->colidx));
    }
    *out = o.release();
    return FGPU_OK;
}

// F: one row per source, at most one entry per row (cond_traverse.rs:600-601); UINT64_MAX = row left empty
static fgpu_info upload_sources(fgpu_ctx* ctx, fgpu_mat** out, const uint64_t* src_ids, uint64_t nsrc, u64 ncols0) {
    std::vector<u32> rp(nsrc + 1), ci;
    ci.reserve(nsrc);
    rp[0] = 0;
    for (u64 i = 0; i < nsrc; ++i) {
        if (src_ids[i] != UINT64_MAX) {
            FGPU_REQUIRE(src_ids[i] < ncols0, FGPU_OUT_OF_BOUNDS, "expand: source %llu = %llu >= %llu",
                         (unsigned long long)i, (unsigned long long)src_ids[i], (unsigned long long)ncols0);
            ci.push_back((u32)src_ids[i]);
        }
        rp[i + 1] = (u32)ci.size();
    }
    MatRef f;
    FGPU_TRY(mat_alloc(ctx, &f.m, nsrc, ncols0, ci.size(), false, 0, false));
    FGPU_TRY(ctx->h2d(f->rowptr, rp.data(), rp.size() * sizeof(u32)));
    if (!ci.empty()) FGPU_TRY(ctx->h2d(f->colidx, ci.data(), ci.size() * sizeof(u32)));
    *out = f.release();
    return FGPU_OK;
}

// The layers of a k-hop chain as the C entries receive them: hop h reads (m[h] \ dm[h]) U dp[h]; `dp` and `dm` are
// nullable as arrays and per hop.
struct Layers {
    const fgpu_mat* const* m;
    const fgpu_mat* const* dp;
    const fgpu_mat* const* dm;
    int nhops;
    const fgpu_mat* dp_at(int h) const { return dp ? dp[h] : nullptr; }
    const fgpu_mat* dm_at(int h) const { return dm ? dm[h] : nullptr; }
};

static fgpu_info check_hops(const Layers& L, uint64_t nsrc) {
    const fgpu_mat* const* m = L.m;
    const int nhops = L.nhops;
    FGPU_REQUIRE(nhops >= 1 && m, FGPU_INVALID, "expand: need at least one hop");
    FGPU_REQUIRE(nsrc < 0xFFFFFFFFull, FGPU_INVALID, "expand: too many source rows");
    for (int h = 0; h < nhops; ++h) {
        const fgpu_mat *dph = L.dp_at(h), *dmh = L.dm_at(h);
        FGPU_REQUIRE(m[h], FGPU_NULL_POINTER, "expand: hop %d base matrix is NULL", h);
        FGPU_REQUIRE(!dph || (dph->nrows == m[h]->nrows && dph->ncols == m[h]->ncols),
                     FGPU_DIM_MISMATCH, "expand: hop %d dp dims differ from m", h);
        FGPU_REQUIRE(!dmh || (dmh->nrows == m[h]->nrows && dmh->ncols == m[h]->ncols),
                     FGPU_DIM_MISMATCH, "expand: hop %d dm dims differ from m", h);
        FGPU_REQUIRE(h == 0 || m[h]->nrows == m[h - 1]->ncols, FGPU_DIM_MISMATCH,
                     "expand: hop %d rows do not match hop %d columns", h, h - 1);
    }
    return FGPU_OK;
}

// ---- first hop from one-entry rows over a clean layer --------------------------------------------------------------------
// F0 has at most one entry per row (cond_traverse.rs:600-601: F[i, src_i] = 1), so F0 x m is "row i = row src_i of m": the
// rows are copied as they are — sorted, unique, nothing to sort or collapse.  The general product (degrees per entry, two
// scans, row offsets, gather, segment lengths, compaction: ~14 launches and three read-backs) is replaced by ONE workgroup that
// scans the <= 4096 source degrees, one read-back of the size, and one copy kernel that also sums the NEXT hop's traversed
// edges (sum over the copied entries of deg_next(col): what mxm_flops would compute for the form decision of hop 2).
constexpr u32 FH_MAX_ROWS = 4096;
__global__ __launch_bounds__(1024) void first_hop_scan_kernel(CsrView f, CsrView m, u32 k, u32* __restrict__ rp, u32* __restrict__ total,
                                                              unsigned long long* __restrict__ tnext_slots) {
    __shared__ u32 s_wave[16];
    __shared__ u32 s_base;
    tnext_slots[threadIdx.x] = 0ull;              // the 64 x 16 words first_hop_copy_kernel sums into (one launch less than a memset)
    u32 d[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                 // thread t owns rows 4 t .. 4 t + 3 (consecutive: the scan stays in order)
        const u32 i = threadIdx.x * 4 + j;
        u32 dg = 0;
        if (i < k && f.rowptr[i + 1] > f.rowptr[i]) {
            u32 b, e;
            row_range(m, f.colidx[f.rowptr[i]], b, e);
            dg = e - b;
        }
        d[j] = dg;
        sum += dg;
    }
    u32 inc = sum;                                 // inclusive scan of the per-thread sums inside the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 v = (u32)__shfl_up((int)inc, o, 64); if ((int)lane_id() >= o) inc += v; }
    if (lane_id() == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int w = 0; w < 16; ++w) { const u32 v = s_wave[w]; s_wave[w] = run; run += v; }
        s_base = run;
    }
    __syncthreads();
    u32 off = s_wave[threadIdx.x >> 6] + inc - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        if (i <= k) rp[i] = off;
        off += d[j];
    }
    if (threadIdx.x == 0) total[0] = s_base;
}
// a lane per RESULT entry (the row of an entry by a search of the <= 4097 row pointers in LDS): a hub source — one :P vertex in
// a thousand has 10^5 out-edges — was copied by ONE wavefront in the first version, 27 us of a 1.45 ms batch.  Sums deg_next
// over the copied column ids (next_rowptr nullable); workgroup 0 also writes the result's row pointers.
__global__ __launch_bounds__(256) void first_hop_copy_kernel(CsrView f, CsrView m, u32 k, const u32* __restrict__ rp, u32 nnz,
                                                             u32* __restrict__ out_rowptr, u32* __restrict__ col,
                                                             const u32* __restrict__ next_rowptr, u32 next_rows,
                                                             unsigned long long* __restrict__ tnext) {
    __shared__ u32 s_rp[FH_MAX_ROWS + 1];
    for (u32 i = threadIdx.x; i <= k; i += 256) {
        const u32 v = rp[i];
        s_rp[i] = v;
        if (blockIdx.x == 0) out_rowptr[i] = v;
    }
    __syncthreads();
    u64 t = 0;
    for (u32 q = blockIdx.x * 256 + threadIdx.x; q < nnz; q += gridDim.x * 256) {
        u32 lo = 0, hi = k - 1;                              // largest row with s_rp[row] <= q
        while (lo < hi) {
            const u32 mid = (lo + hi + 1) >> 1;
            if (s_rp[mid] <= q) lo = mid; else hi = mid - 1;
        }
        u32 b, e;
        row_range(m, f.colidx[f.rowptr[lo]], b, e);
        const u32 c = m.colidx[b + (q - s_rp[lo])];
        col[q] = c;
        if (next_rowptr && c < next_rows) t += next_rowptr[c + 1] - next_rowptr[c];
    }
    if (tnext) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
        const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
        if (lane_id() == 0 && t) atomicAdd(&tnext[(wave & 63u) * 16u], (unsigned long long)t);   // 64 slots, a 128-byte line apart
    }
}
// the 64 slots summed; lane 0 publishes the sum into the lane's mapped line itself when there is one (ctx.hip pub_begin)
__global__ void first_hop_fold_kernel(unsigned long long* __restrict__ tnext, u32* __restrict__ pub, u32 seq) {
    u64 v = tnext[(size_t)threadIdx.x * 16];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if (threadIdx.x == 0) {
        if (pub) {
            __hip_atomic_store(pub + 0, (u32)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(pub + 1, (u32)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(pub + 15, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            tnext[1] = v;
        }
    }
}

// *out = F0 x m for a clean hop (no dp / dm); *T0 = its traversed edges; *Tnext (when `next` is a plain CSR) = the traversed
// edges of the following hop over `next`.  Returns FGPU_NO_VALUE when the shortcut does not apply (the caller takes the general path).
static fgpu_info first_hop_rows(fgpu_ctx* ctx, const fgpu_mat* f, const fgpu_mat* m, const fgpu_mat* next, fgpu_mat** out,
                                u64* T0, u64* Tnext, bool* have_next) {
    *have_next = false;
    const u32 k = (u32)f->nrows;
    // (k == FH_MAX_ROWS is out: the scan kernel's 1024 threads x 4 rows write rp[0 .. 4095], never rp[4096])
    if (k == 0 || k >= FH_MAX_ROWS || f->is_hyper() || f->nnz > f->nrows || m->nnz == 0 || f->nnz == 0) return FGPU_NO_VALUE;
    DevBuf<u32> rp, tot;
    DevBuf<u64> tn;
    FGPU_TRY(rp.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(tot.alloc(ctx, 1));
    FGPU_TRY(tn.alloc(ctx, 64 * 16));
    FGPU_TRY(launch(first_hop_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream(), view_of(f), view_of(m), k, rp.p, tot.p,
                    (unsigned long long*)tn.p));
    u32 nnz = 0;
    FGPU_TRY(read_u32(ctx, tot.p, &nnz));
    *T0 = nnz;
    MatRef c;
    FGPU_TRY(mat_alloc(ctx, &c.m, k, m->ncols, nnz, false, 0, false));
    const bool sum_next = next && !next->is_hyper() && next->nnz && nnz;
    fgpu_info i = FGPU_OK;
    {
        ProfScope ps(ctx, "first_hop_copy_kernel", 4 * ((u64)k + 1) + 8 * (u64)nnz);   // the row pointers, every entry read + written
        u32 grid = cdiv(nnz ? nnz : 1, 256 * 4);
        if (grid > (u32)ctx->cus * 4) grid = ctx->cus * 4;
        i = launch(first_hop_copy_kernel, dim3(grid ? grid : 1), dim3(256), 0, ctx->stream(), view_of(f), view_of(m), k,
                   (const u32*)rp.p, nnz, c->rowptr, c->colidx, sum_next ? (const u32*)next->rowptr : (const u32*)nullptr,
                   sum_next ? (u32)next->nrows : 0u, sum_next ? (unsigned long long*)tn.p : (unsigned long long*)nullptr);
    }
    if (i == FGPU_OK && sum_next) {
        u32* pub = nullptr;
        u32 seq = 0;
        const bool mapped = pub_begin(ctx, &pub, &seq);
        i = launch(first_hop_fold_kernel, dim3(1), dim3(64), 0, ctx->stream(), (unsigned long long*)tn.p, mapped ? pub : (u32*)nullptr, seq);
        if (i == FGPU_OK && mapped) {
            u32 w[2] = {0, 0};
            i = pub_wait(ctx, seq, 2, w);
            *Tnext = (u64)w[0] | ((u64)w[1] << 32);
        } else if (i == FGPU_OK) {
            i = read_u64(ctx, tn.p + 1, Tnext);
        }
        *have_next = i == FGPU_OK;
    }
    if (i != FGPU_OK) { if (i == FGPU_DEVICE) set_error("first hop: device call failed"); return i; }
    *out = c.release();
    return FGPU_OK;
}

// ---- the first hop from one-entry rows over DIRTY layers -----------------------------------------------------------------
// Row i of F holds one source u: (F·m)<not (F·dm)> U (F·dp) is then (m[u] \ dm[u]) U dp[u] row by row (the row-level mask of
// Matrix::delta_lmxm, matrix.rs:1343-1361, is the row's own tombstones).  The general product does this in ~75 launches of a
// few microseconds (three gathers, three sorts, the merge machinery); here: candidate offsets (one single-workgroup scan), keep
// flags a lane per candidate (binary searches in the sorted rows), two scans of the flags, row lengths, and a fill that places
// every kept candidate by its rank among the kept entries of both lists — the result row stays ascending and unique whatever
// the layers hold (no Delta invariant is assumed: a dp entry that m already has is dropped, a tombstone outside m does nothing).
__global__ __launch_bounds__(1024) void fhd_scan_kernel(CsrView f, CsrView m, CsrView dp, u32 k, u32* __restrict__ cm, u32* __restrict__ cp,
                                                        u32* __restrict__ totals, unsigned long long* __restrict__ tnext_slots) {
    __shared__ u32 s_wave[2][16];
    tnext_slots[threadIdx.x] = 0ull;
    u32 a[4], b[4], sa = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        u32 da = 0, db = 0;
        if (i < k && f.rowptr[i + 1] > f.rowptr[i]) {
            const u32 u = f.colidx[f.rowptr[i]];
            u32 x, y;
            row_range(m, u, x, y); da = y - x;
            row_range(dp, u, x, y); db = y - x;
        }
        a[j] = da; b[j] = db; sa += da; sb += db;
    }
    u32 ia = sa, ib = sb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 va = (u32)__shfl_up((int)ia, o, 64), vb = (u32)__shfl_up((int)ib, o, 64);
        if ((int)lane_id() >= o) { ia += va; ib += vb; }
    }
    if (lane_id() == 63) { s_wave[0][threadIdx.x >> 6] = ia; s_wave[1][threadIdx.x >> 6] = ib; }
    __syncthreads();
    if (threadIdx.x < 2) {
        u32 run = 0;
        for (int w = 0; w < 16; ++w) { const u32 v = s_wave[threadIdx.x][w]; s_wave[threadIdx.x][w] = run; run += v; }
        totals[threadIdx.x] = run;
    }
    __syncthreads();
    u32 oa = s_wave[0][threadIdx.x >> 6] + ia - sa, ob = s_wave[1][threadIdx.x >> 6] + ib - sb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        if (i <= k) { cm[i] = oa; cp[i] = ob; }
        oa += a[j]; ob += b[j];
    }
}
__device__ __forceinline__ u32 fhd_lower_bound(const u32* __restrict__ col, u32 b, u32 e, u32 x) {
    while (b < e) {
        const u32 mid = (b + e) >> 1;
        if (col[mid] < x) b = mid + 1; else e = mid;
    }
    return b;
}
// the row of candidate q: largest i with ptr[i] <= q (k + 1 offsets in LDS)
__device__ __forceinline__ u32 fhd_row_of(const u32* s_ptr, u32 k, u32 q) {
    u32 lo = 0, hi = k - 1;
    while (lo < hi) {
        const u32 mid = (lo + hi + 1) >> 1;
        if (s_ptr[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// FILL = false: keep flags.  FILL = true: every kept candidate to its place (rank among the kept entries of both lists).
template <bool FILL>
__global__ __launch_bounds__(256) void fhd_cand_kernel(CsrView f, CsrView m, CsrView dp, CsrView dm, u32 k, const u32* __restrict__ cm,
                                                       const u32* __restrict__ cp, u32 ncm, u32 ncp, u32* __restrict__ keepm,
                                                       u32* __restrict__ keepp, const u32* __restrict__ pm, const u32* __restrict__ pp,
                                                       const u32* __restrict__ rowptr, u32* __restrict__ col,
                                                       const u32* __restrict__ next_rowptr, u32 next_rows,
                                                       unsigned long long* __restrict__ tnext) {
    __shared__ u32 s_cm[FH_MAX_ROWS + 1], s_cp[FH_MAX_ROWS + 1];
    for (u32 i = threadIdx.x; i <= k; i += 256) { s_cm[i] = cm[i]; s_cp[i] = cp[i]; }
    __syncthreads();
    u64 t = 0;
    for (u32 q = blockIdx.x * 256 + threadIdx.x; q < ncm + ncp; q += gridDim.x * 256) {
        const bool from_m = q < ncm;
        const u32 c = from_m ? q : q - ncm;
        const u32 i = fhd_row_of(from_m ? s_cm : s_cp, k, c);
        const u32 u = f.colidx[f.rowptr[i]];
        u32 mb, me, pb, pe, db, de;
        row_range(m, u, mb, me);
        row_range(dp, u, pb, pe);
        row_range(dm, u, db, de);
        const u32 j = c - (from_m ? s_cm[i] : s_cp[i]);
        const u32 x = from_m ? m.colidx[mb + j] : dp.colidx[pb + j];
        const u32 dl = fhd_lower_bound(dm.colidx, db, de, x);
        const bool tomb = dl < de && dm.colidx[dl] == x;
        bool keep;
        u32 other = 0;                                       // index of x's lower bound in the OTHER list
        if (from_m) {
            keep = !tomb;
            if (FILL) other = fhd_lower_bound(dp.colidx, pb, pe, x) - pb;
        } else {
            const u32 ml = fhd_lower_bound(m.colidx, mb, me, x);
            keep = !(ml < me && m.colidx[ml] == x && !tomb);  // (m keeps x itself: the dp copy is a duplicate)
            other = ml - mb;
        }
        if (!FILL) {
            (from_m ? keepm : keepp)[c] = keep ? 1u : 0u;
        } else if (keep) {
            const u32 pos = from_m ? (pm[c] - pm[s_cm[i]]) + (pp[s_cp[i] + other] - pp[s_cp[i]])
                                   : (pp[c] - pp[s_cp[i]]) + (pm[s_cm[i] + other] - pm[s_cm[i]]);
            col[rowptr[i] + pos] = x;
            if (next_rowptr && x < next_rows) t += next_rowptr[x + 1] - next_rowptr[x];
        }
    }
    if (FILL && tnext) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
        const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
        if (lane_id() == 0 && t) atomicAdd(&tnext[(wave & 63u) * 16u], (unsigned long long)t);
    }
}
// row lengths from the two flag scans, their exclusive scan, the total published (k <= 4095)
__global__ __launch_bounds__(1024) void fhd_rowptr_kernel(const u32* __restrict__ cm, const u32* __restrict__ cp, const u32* __restrict__ pm,
                                                          const u32* __restrict__ pp, u32 k, u32* __restrict__ rowptr, u32* __restrict__ pub,
                                                          u32 seq, u32* __restrict__ total) {
    __shared__ u32 s_wave[16];
    u32 d[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        d[j] = i < k ? (pm[cm[i + 1]] - pm[cm[i]]) + (pp[cp[i + 1]] - pp[cp[i]]) : 0u;
        sum += d[j];
    }
    u32 inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 v = (u32)__shfl_up((int)inc, o, 64); if ((int)lane_id() >= o) inc += v; }
    if (lane_id() == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int w = 0; w < 16; ++w) { const u32 v = s_wave[w]; s_wave[w] = run; run += v; }
    }
    __syncthreads();
    u32 off = s_wave[threadIdx.x >> 6] + inc - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        if (i <= k) rowptr[i] = off;
        if (i == k) {
            total[0] = off;
            if (pub) {
                __hip_atomic_store(pub + 0, off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(pub + 15, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        off += d[j];
    }
}

static fgpu_info first_hop_rows_dirty(fgpu_ctx* ctx, const fgpu_mat* f, const fgpu_mat* m, const fgpu_mat* dp, const fgpu_mat* dm,
                                      const fgpu_mat* next, fgpu_mat** out, u64* T0, u64* Tnext, bool* have_next) {
    *have_next = false;
    const u32 k = (u32)f->nrows;
    if (k == 0 || k >= FH_MAX_ROWS || f->is_hyper() || f->nnz > f->nrows || f->nnz == 0 || m->is_hyper()) return FGPU_NO_VALUE;
    hipStream_t st = ctx->stream();
    DevBuf<u32> cm, cp, tot, empty;
    DevBuf<u64> tn;
    FGPU_TRY(cm.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(cp.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(tot.alloc(ctx, 4));
    FGPU_TRY(tn.alloc(ctx, 64 * 16));
    FGPU_TRY(empty.alloc(ctx, 4));
    FGPU_HIP(hipMemsetAsync(empty.p, 0, 4 * sizeof(u32), st));
    auto view_or_empty = [&](const fgpu_mat* a) {
        if (a && a->nnz) return view_of(a);
        CsrView v;                                           // hypersparse with no stored row: every row_range is empty
        v.rowptr = empty.p; v.colidx = empty.p; v.hrows = empty.p; v.nvec = 0; v.nrows = (u32)m->nrows;
        return v;
    };
    const CsrView vm = view_of(m), vdp = view_or_empty(dp), vdm = view_or_empty(dm), vf = view_of(f);
    FGPU_TRY(launch(fhd_scan_kernel, dim3(1), dim3(1024), 0, st, vf, vm, vdp, k, cm.p, cp.p, tot.p, (unsigned long long*)tn.p));
    u32 w2[2] = {0, 0};
    FGPU_TRY(read_words(ctx, tot.p, 2, w2));
    const u32 ncm = w2[0], ncp = w2[1];
    *T0 = (u64)ncm + ncp;                                    // traversed edges of the hop: deg over m and over dp
    DevBuf<u32> keepm, keepp, pm, pp;
    FGPU_TRY(keepm.alloc(ctx, (size_t)ncm + 1)); FGPU_TRY(keepp.alloc(ctx, (size_t)ncp + 1));
    FGPU_TRY(pm.alloc(ctx, (size_t)ncm + 1)); FGPU_TRY(pp.alloc(ctx, (size_t)ncp + 1));
    u32 grid = cdiv((u64)ncm + ncp ? (u64)ncm + ncp : 1, 256 * 2);
    if (grid > (u32)ctx->cus * 4) grid = ctx->cus * 4;
    FGPU_HIP(hipMemsetAsync(keepm.p + ncm, 0, sizeof(u32), st));
    FGPU_HIP(hipMemsetAsync(keepp.p + ncp, 0, sizeof(u32), st));
    {
        ProfScope ps(ctx, "fhd_cand_kernel", 0);
        FGPU_TRY(launch(fhd_cand_kernel<false>, dim3(grid ? grid : 1), dim3(256), 0, st, vf, vm, vdp, vdm, k, (const u32*)cm.p, (const u32*)cp.p,
                        ncm, ncp, keepm.p, keepp.p, (const u32*)nullptr, (const u32*)nullptr, (const u32*)nullptr, (u32*)nullptr,
                        (const u32*)nullptr, 0u, (unsigned long long*)nullptr));
    }
    FGPU_TRY(scan_u32(ctx, keepm.p, pm.p, (u64)ncm + 1, nullptr));
    FGPU_TRY(scan_u32(ctx, keepp.p, pp.p, (u64)ncp + 1, nullptr));
    DevBuf<u32> rp;
    FGPU_TRY(rp.alloc(ctx, (size_t)k + 1));
    u32 nnz = 0;
    {
        u32* pub = nullptr;
        u32 seq = 0;
        const bool mapped = pub_begin(ctx, &pub, &seq);
        FGPU_TRY(launch(fhd_rowptr_kernel, dim3(1), dim3(1024), 0, st, (const u32*)cm.p, (const u32*)cp.p, (const u32*)pm.p,
                        (const u32*)pp.p, k, rp.p, mapped ? pub : (u32*)nullptr, seq, tot.p + 2));
        if (mapped) { u32 w[1] = {0}; FGPU_TRY(pub_wait(ctx, seq, 1, w)); nnz = w[0]; }
        else FGPU_TRY(read_u32(ctx, tot.p + 2, &nnz));
    }
    MatRef c;
    FGPU_TRY(mat_alloc(ctx, &c.m, k, m->ncols, nnz, false, 0, false));
    const bool sum_next = next && !next->is_hyper() && next->nnz && nnz;
    fgpu_info i = FGPU_OK;
    if (hipMemcpyAsync(c->rowptr, rp.p, ((size_t)k + 1) * sizeof(u32), hipMemcpyDeviceToDevice, st) != hipSuccess) i = FGPU_DEVICE;
    if (i == FGPU_OK && nnz) {
        i = launch(fhd_cand_kernel<true>, dim3(grid ? grid : 1), dim3(256), 0, st, vf, vm, vdp, vdm, k, (const u32*)cm.p,
                   (const u32*)cp.p, ncm, ncp, (u32*)nullptr, (u32*)nullptr, (const u32*)pm.p, (const u32*)pp.p, (const u32*)rp.p,
                   c->colidx, sum_next ? (const u32*)next->rowptr : (const u32*)nullptr, sum_next ? (u32)next->nrows : 0u,
                   sum_next ? (unsigned long long*)tn.p : (unsigned long long*)nullptr);
    }
    if (i == FGPU_OK && sum_next) {
        u32* pub = nullptr;
        u32 seq = 0;
        const bool mapped = pub_begin(ctx, &pub, &seq);
        i = launch(first_hop_fold_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)tn.p, mapped ? pub : (u32*)nullptr, seq);
        if (i == FGPU_OK && mapped) {
            u32 w[2] = {0, 0};
            i = pub_wait(ctx, seq, 2, w);
            *Tnext = (u64)w[0] | ((u64)w[1] << 32);
        } else if (i == FGPU_OK) {
            i = read_u64(ctx, tn.p + 1, Tnext);
        }
        *have_next = i == FGPU_OK;
    }
    if (i != FGPU_OK) { if (i == FGPU_DEVICE) set_error("dirty first hop: device call failed"); return i; }
    *out = c.release();
    return FGPU_OK;
}

// ---- dropping the empty source rows of a count-only chain before it goes to bits ------------------------------------------
// A source without out-edges (half of the vertices of an R-MAT graph, half of a `:P` batch) leaves an empty row after the
// first hop and can never contribute again, but keeps its bit in every 128-byte row of the bit state.  When the live rows
// fit HALF the words (1024 sources, 499 live: 16 -> 8 words per vertex) the frontier is renumbered to the live rows only:
// the dense last hop gathers 64-byte rows (two vertices per line, a state that fits the Infinity Cache at RMAT-22: -13 %),
// the middle hop writes half the bytes (-27 %).  The way back: the checksum's row hashes go through `map`, the emitted
// row pointers through `rank` (bp_to_csr).
__global__ void cr_flag_kernel(const u32* __restrict__ rowptr, u32 k, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= k) flag[i] = (i < k && rowptr[i + 1] > rowptr[i]) ? 1u : 0u;
}
// k <= 4096 rows (a child batch holds 1024): flags, their exclusive scan and the read-back of the live count in ONE
// single-workgroup launch (was: flag kernel, scan, a one-thread publish kernel)
__global__ __launch_bounds__(1024) void cr_rank_kernel(const u32* __restrict__ rowptr, u32 k, u32* __restrict__ rank, u32* __restrict__ pub,
                                                       u32 seq) {
    __shared__ u32 s_wave[16];
    u32 d[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        d[j] = (i < k && rowptr[i + 1] > rowptr[i]) ? 1u : 0u;
        sum += d[j];
    }
    u32 inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 v = (u32)__shfl_up((int)inc, o, 64); if ((int)lane_id() >= o) inc += v; }
    if (lane_id() == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int w = 0; w < 16; ++w) { const u32 v = s_wave[w]; s_wave[w] = run; run += v; }
    }
    __syncthreads();
    u32 off = s_wave[threadIdx.x >> 6] + inc - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 i = threadIdx.x * 4 + j;
        if (i <= k) rank[i] = off;
        if (i == k && pub) {
            __hip_atomic_store(pub + 0, off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(pub + 15, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        off += d[j];
    }
}
__global__ void cr_build_kernel(const u32* __restrict__ rowptr, const u32* __restrict__ colidx, u32 k, u32 nnz, const u32* __restrict__ rank,
                                u32* __restrict__ new_rowptr, u32* __restrict__ new_colidx, u32* __restrict__ map, u32 nlive) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k && rowptr[i + 1] > rowptr[i]) { new_rowptr[rank[i]] = rowptr[i]; map[rank[i]] = i; }
    if (i == k) new_rowptr[nlive] = rowptr[k];
    for (u32 q = i; q < nnz; q += gridDim.x * blockDim.x) new_colidx[q] = colidx[q];   // (the entries stay where they are)
}
static u32 bits_stride(u32 rows) {                         // = bp_layout's row stride for `rows` source rows
    u32 w = (rows + 63) / 64;
    if (w == 0) w = 1;
    if (w > 64) return ((w + 63) / 64) * 64;
    u32 p = 1;
    while (p < w) p <<= 1;
    return p;
}
// *out = f without its empty rows (nullptr: nothing to gain, f stays), map[new row] = old row
static fgpu_info compact_source_rows(fgpu_ctx* ctx, const fgpu_mat* f, fgpu_mat** out, DevBuf<u32>& map, DevBuf<u32>& rank_out) {
    *out = nullptr;
    const u32 k = (u32)f->nrows;
    if (f->is_hyper() || k < 128 || f->nnz == 0) return FGPU_OK;
    DevBuf<u32> flag, rank;
    FGPU_TRY(rank.alloc(ctx, (size_t)k + 1));
    u32 nlive = 0;
    u32* pub = nullptr;
    u32 seq = 0;
    if (k <= 4095 && pub_begin(ctx, &pub, &seq)) {
        FGPU_TRY(launch(cr_rank_kernel, dim3(1), dim3(1024), 0, ctx->stream(), (const u32*)f->rowptr, k, rank.p, pub, seq));
        u32 w[1] = {0};
        FGPU_TRY(pub_wait(ctx, seq, 1, w));
        nlive = w[0];
    } else {
        FGPU_TRY(flag.alloc(ctx, (size_t)k + 1));
        FGPU_TRY(launch(cr_flag_kernel, dim3(cdiv((u64)k + 1, 256)), dim3(256), 0, ctx->stream(), (const u32*)f->rowptr, k, flag.p));
        FGPU_TRY(scan_u32(ctx, flag.p, rank.p, (u64)k + 1, nullptr));
        FGPU_TRY(read_u32(ctx, rank.p + k, &nlive));
    }
    if (nlive == 0 || bits_stride(nlive) >= bits_stride(k)) return FGPU_OK;
    MatRef c;
    FGPU_TRY(mat_alloc(ctx, &c.m, nlive, f->ncols, f->nnz, false, 0, false));
    FGPU_TRY(map.alloc(ctx, nlive));
    u32 grid = cdiv((u64)k + 1, 256);
    const u32 want = cdiv(f->nnz, 256 * 8);
    if (grid < want) grid = want < (u32)ctx->cus * 4 ? want : (u32)ctx->cus * 4;
    {
        ProfScope ps(ctx, "cr_build_kernel", 12 * ((u64)k + 1) + 8 * (u64)f->nnz);   // row pointers, ranks, map; the entries read + written
        FGPU_TRY(launch(cr_build_kernel, dim3(grid), dim3(256), 0, ctx->stream(), (const u32*)f->rowptr, (const u32*)f->colidx, k,
                        (u32)f->nnz, (const u32*)rank.p, c->rowptr, c->colidx, map.p, nlive));
    }
    rank_out = std::move(rank);        // rank[i] = live rows before source row i, rank[k] = nlive: the way back (bp_to_csr)
    *out = c.release();
    return FGPU_OK;
}

// One pass of a whole-frontier call (expand_count_scan below): F is already on the device — one entry per row, no empty
// rows — and row i of it is row rowmap[i] of the CALL (what the checksum's row hashes need).
struct ChainSources {
    MatRef f;                        // taken over by the chain
    DevBuf<u32>* rowmap = nullptr;   // moved into the bit state while the chain runs, handed back when it ends in CSR form
    DevBuf<u64>* rowhash = nullptr;  // nullable: the hash of every row, for rows that stand for classes of call rows; moved like rowmap
};

// the caller's destination-label bitmap (one bit per column; nullptr: no filter, bm.p stays nullptr) on the device
static fgpu_info label_to_device(fgpu_ctx* ctx, const uint64_t* host_bitmap, u64 ncols, DevBuf<u64>& bm) {
    if (!host_bitmap) return FGPU_OK;
    const u64 nw = (ncols + 63) / 64;
    FGPU_TRY(bm.alloc(ctx, nw + 1));
    return ctx->h2d(bm.p, host_bitmap, nw * sizeof(u64));
}

// What a chain is asked for, and what it hands back.  A chain runs on sorted-CSR products until a hop is cheaper in bit form
// and stays there; the END says what the caller wants of the form it finished in:
//   Csr            the result as a snapshot, whatever form the chain ended in (ChainResult::Csr);
//   Count(+Sum)    nnz (and the checksum): a chain in bit form counts there and builds no CSR (ChainResult::Counts), one
//                  that stayed in CSR form hands that CSR back for the caller to count (ChainResult::Csr);
//   Bits           a chain in bit form hands its state over (ChainResult::Bits), one in CSR form its CSR (ChainResult::Csr).
enum class ChainEnd { Csr, Count, CountSum, Bits };
struct ChainRequest {
    const uint64_t* src_ids;          // one source per row, UINT64_MAX = the row stays empty (unused with `pre`)
    uint64_t nsrc;
    Layers L;
    const uint64_t* label;            // destination-label bitmap on the host, nullable
    u64* flops;                       // nullable: += the traversed edges
    ChainEnd end;
    ChainSources* pre = nullptr;      // the sources are on the device already
    bool counting() const { return end == ChainEnd::Count || end == ChainEnd::CountSum; }
};
struct ChainResult {
    enum Kind { None, Csr, Counts, Bits } kind = None;
    MatRef mat;                       // Csr
    u64 nnz = 0, checksum = 0;        // Counts (checksum only for ChainEnd::CountSum)
    BitState bits;                    // Bits
};

// the running state of one chain: the frontier as a CSR `f`, or (once `bits`) as the bit state `bs`
struct Chain {
    MatRef f;
    bool bits = false;
    BitState bs;
    u64 T_known = 0;                      // traversed edges of T_f over T_for, when an earlier step already summed them
    const fgpu_mat *T_for = nullptr, *T_f = nullptr;
};

// The first hop from one-entry rows: the source rows of m copied over a clean layer (first_hop_rows above),
// (m[u] \ dm[u]) U dp[u] row by row over dirty ones (first_hop_rows_dirty).  *done = false: the shortcut does not apply.
static fgpu_info chain_first_hop(fgpu_ctx* ctx, const ChainRequest& rq, Chain& ch, bool* done) {
    const Layers& L = rq.L;
    const fgpu_mat *dph = L.dp_at(0), *dmh = L.dm_at(0), *next = L.nhops > 1 ? L.m[1] : nullptr;
    const bool clean = !(dph && dph->nnz) && !(dmh && dmh->nnz);
    MatRef c;
    u64 T0 = 0, Tn = 0;
    bool have = false;
    const fgpu_info fi = clean ? first_hop_rows(ctx, ch.f.get(), L.m[0], next, &c.m, &T0, &Tn, &have)
                               : first_hop_rows_dirty(ctx, ch.f.get(), L.m[0], dph, dmh, next, &c.m, &T0, &Tn, &have);
    *done = fi == FGPU_OK;
    if (fi == FGPU_NO_VALUE) return FGPU_OK;
    FGPU_TRY(fi);
    // (a first hop heavy enough for the bit form — T0 * ratio > nnz — is a batch of hub sources; it is still
    // correct as a copy, and the next hop's decision sees its true volume)
    if (rq.flops) *rq.flops += T0;
    ch.f = std::move(c);
    // (over dirty layers: the next hop's traversed edges over its BASE matrix only — with a dirty next layer its dp part is
    // summed there)
    if (have) { ch.T_known = Tn; ch.T_for = L.m[1]; ch.T_f = ch.f.get(); }
    return FGPU_OK;
}

// Hop h of a chain still in CSR form: does it leave that form here?  Hops run on the sorted-CSR products until a hop's
// gather volume T makes the bit-parallel form cheaper (bitexpand.hip): it costs one pass over A' gathering max(64, 8 W)
// bytes per entry, whatever T is; the CSR product moves ~T entries several times.  Once dense, stay dense.
// On return ch.bits says whether it left; *hop_done, that hop h itself is done as well (the push).
static fgpu_info chain_leave_csr(fgpu_ctx* ctx, const ChainRequest& rq, Chain& ch, int h, bool* hop_done) {
    *hop_done = false;
    const int mode = ctx->opt.expand_mode;
    const fgpu_mat *mh = rq.L.m[h], *dph = rq.L.dp_at(h), *dmh = rq.L.dm_at(h);
    if (mode == 1 || mh->is_hyper() || !mh->nnz || mh->nnz >= 0x7FFFFFFFull || !ch.f->nnz) return FGPU_OK;
    const u64 w = (rq.nsrc + 63) / 64;
    const u64 mem = 2ull * (mh->nrows > mh->ncols ? mh->nrows : mh->ncols) * (w <= 64 ? 2 * w : w + 64) * 8;
    bool go = (mode == 2);
    u64 T = 0;
    if ((mode == 0 && mem < (64ull << 30)) || go) {
        if (ch.T_for == mh && ch.T_f == ch.f.get()) T = ch.T_known;          // summed while the first hop's rows were copied
        else FGPU_TRY(mxm_flops(ctx, ch.f.get(), mh, &T));
        // measured: a sorted-CSR hop costs ~0.12-0.16 ns per gathered entry (RMAT-22: 6 ms at T = 36 M; RMAT-26:
        // 12 ms at T ~ 100 M), the first bit hop — the sparse pull, a flag probe per entry of A' — 5.5-6 ps per matrix
        // entry whatever the row width (1.45 ms at RMAT-24, 6.2 ms at RMAT-26): the chain leaves the CSR form once
        // T exceeds ~ nnz / 28.  (The round-1 rule, T * 1024 > nnz * row_bytes = nnz / 8 at 1024 rows, dated from a
        // 41 ps-per-entry pull and kept RMAT-26 batches in an 8.7 ms sort.)
        if (mode == 0) go = T * ctx->opt.expand_bits_ratio > mh->nnz;
    }
    if (!go) return FGPU_OK;
    if (ctx->opt.expand_compact && !rq.pre) {
        // the empty source rows stay behind (compact_source_rows above); bp_to_csr finds the way back
        MatRef fc;
        const u32 k_full = (u32)ch.f->nrows;
        FGPU_TRY(compact_source_rows(ctx, ch.f.get(), &fc.m, ch.bs.rowmap, ch.bs.rowrank));
        if (fc.get()) { ch.f = std::move(fc); ch.bs.nsrc_full = k_full; }
    }
    // leaving the CSR form: a frontier whose out-edges are FEW beside the matrix is pushed into the bit state
    // (one 8-byte atomic per traversed edge: measured ~8 G/s on random words of a 2 GiB state — 33 M edges
    // took 4.06 ms where the sparse pull takes 2.64 ms, so the bar is a 32nd of the matrix, not a quarter),
    // a heavier one is scattered to a dense X and pulled
    if (T * 32 <= mh->nnz) {
        if (rq.flops) {
            *rq.flops += T;
            if (dph && dph->nnz) {
                u64 Tp = 0;
                FGPU_TRY(mxm_flops(ctx, ch.f.get(), dph, &Tp));
                *rq.flops += Tp;
            }
        }
        FGPU_TRY(bp_push_from_csr(ctx, ch.bs, ch.f.get(), mh, dph, dmh));
        ch.f.reset();
        ch.bits = true;
        *hop_done = true;
        return FGPU_OK;
    }
    FGPU_TRY(bp_from_csr(ctx, ch.bs, ch.f.get()));
    ch.f.reset();
    ch.bs.pre_for = mh;                    // T is this hop's traversed-edge count over mh: no need to sum it again
    ch.bs.pre_flops = T;
    ch.bits = true;
    return FGPU_OK;
}

// the last hop of a counting chain in bit form counts its rows where they are produced: no result state is written,
// zeroed or read back (bitexpand.hip bp_hop_count)
static fgpu_info chain_count_hop(fgpu_ctx* ctx, const ChainRequest& rq, Chain& ch, int h, ChainResult& out) {
    const fgpu_mat* mh = rq.L.m[h];
    DevBuf<u64> bm;
    FGPU_TRY(label_to_device(ctx, rq.label, mh->ncols, bm));
    FGPU_TRY(bp_hop_count(ctx, ch.bs, mh, rq.L.dp_at(h), rq.L.dm_at(h), rq.flops, bm.p, &out.nnz,
                          rq.end == ChainEnd::CountSum ? &out.checksum : nullptr));
    out.kind = ChainResult::Counts;
    return FGPU_OK;
}

// every hop is done: the form the chain is in, turned into what the request's end asks for
static fgpu_info chain_end(fgpu_ctx* ctx, const ChainRequest& rq, Chain& ch, ChainResult& out) {
    if (ch.bits && rq.end == ChainEnd::Bits) {
        out.bits = std::move(ch.bs);
        out.kind = ChainResult::Bits;
        return FGPU_OK;
    }
    if (ch.bits) {
        DevBuf<u64> bm;
        FGPU_TRY(label_to_device(ctx, rq.label, ch.bs.n, bm));
        if (rq.counting()) {
            FGPU_TRY(bp_count(ctx, ch.bs, bm.p, &out.nnz, rq.end == ChainEnd::CountSum ? &out.checksum : nullptr));
            out.kind = ChainResult::Counts;
        } else {
            FGPU_TRY(bp_to_csr(ctx, ch.bs, bm.p, &out.mat.m));
            out.kind = ChainResult::Csr;
        }
        bp_finish(ctx, ch.bs);   // the next batch's state finds a zeroed block instead of a 2 GiB memset
        return FGPU_OK;
    }
    if (rq.label) {
        DevBuf<u64> bm;
        FGPU_TRY(label_to_device(ctx, rq.label, ch.f->ncols, bm));
        MatRef c;
        FGPU_TRY(filter_by_bitmap(ctx, &c.m, ch.f.get(), bm.p));
        if (hipStreamSynchronize(ctx->stream()) != hipSuccess) return FGPU_DEVICE;
        ch.f = std::move(c);
    }
    if (rq.pre && rq.pre->rowmap) *rq.pre->rowmap = std::move(ch.bs.rowmap);
    if (rq.pre && rq.pre->rowhash) *rq.pre->rowhash = std::move(ch.bs.rowhash);
    out.mat = std::move(ch.f);
    out.kind = ChainResult::Csr;
    return FGPU_OK;
}

// the k-hop chain every fgpu_expand* entry runs: the result stays on the device
static fgpu_info expand_device(fgpu_ctx* ctx, const ChainRequest& rq, ChainResult& out) {
    const Layers& L = rq.L;
    Chain ch;
    if (rq.pre) {
        ch.f = std::move(rq.pre->f);
        if (rq.pre->rowmap) ch.bs.rowmap = std::move(*rq.pre->rowmap);
        if (rq.pre->rowhash) ch.bs.rowhash = std::move(*rq.pre->rowhash);
    } else {
        FGPU_TRY(check_hops(L, rq.nsrc));
        FGPU_TRY(upload_sources(ctx, &ch.f.m, rq.src_ids, rq.nsrc, L.m[0]->nrows));
    }
    const bool fused_count = rq.counting() && ctx->opt.expand_fuse_count;
    for (int h = 0; h < L.nhops; ++h) {
        if (h == 0 && ctx->opt.expand_mode != 2 && ctx->opt.expand_first_hop) {
            bool done = false;
            FGPU_TRY(chain_first_hop(ctx, rq, ch, &done));
            if (done) continue;
        }
        if (!ch.bits) {
            bool hop_done = false;
            FGPU_TRY(chain_leave_csr(ctx, rq, ch, h, &hop_done));
            if (hop_done) continue;
        }
        if (ch.bits) {
            if (fused_count && h == L.nhops - 1) return chain_count_hop(ctx, rq, ch, h, out);
            // (the hop right before a counting end of the chain writes its state in the layout that end gathers from)
            FGPU_TRY(bp_hop(ctx, ch.bs, L.m[h], L.dp_at(h), L.dm_at(h), rq.flops, (rq.flops && h + 1 < L.nhops) ? L.m[h + 1] : nullptr,
                            (fused_count && h + 2 == L.nhops) ? L.m[h + 1] : nullptr));
            continue;
        }
        MatRef c;
        FGPU_TRY(delta_lmxm_device(ctx, &c.m, ch.f.get(), L.m[h], L.dp_at(h), L.dm_at(h), rq.flops));
        ch.f = std::move(c);
    }
    return chain_end(ctx, rq, ch, out);
}

// ---- exact trail counts for k <= 2 -------------------------------------------------------------
// The reference evaluates `[*1..k]` with a per-row DFS over TRAILS (edge-unique paths, one row per path:
// CondVarLenTraverseOp, cond_var_len_traverse.rs:196-387).  For k <= 2 the number of trails between two nodes is a
// counting product over the effective adjacency: length 1 = the pair's multiplicity; length 2 = sum over the
// intermediates m of w(a, m) * w(m, b) — PLUS_PAIR on pattern matrices, PLUS_TIMES when the matrices carry per-pair
// multiplicities — minus the walks that use ONE edge twice, which at length 2 can only be a self-loop a -> a -> a
// (w(a, a) of them).  From k = 3 on walks that revisit an edge no longer have a product form, so the DFS stays.
__global__ __launch_bounds__(256) void row_weight_kernel(CsrView c1, CsrView a, const u64* __restrict__ aw,
                                                        const u32* __restrict__ src, u32 nrows, u64* __restrict__ w1) {
    // C1 = F0 x A with one source per row: row i of C1 IS row src[i] of A, entry for entry
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    for (u32 i = wave; i < nrows; i += nwaves) {
        const u32 cb = c1.rowptr[i], ce = c1.rowptr[i + 1];
        if (cb == ce) continue;
        u32 ab, ae;
        row_range(a, src[i], ab, ae);
        for (u32 k = lane; k < ce - cb; k += 64) w1[cb + k] = aw ? aw[ab + k] : 1ull;
    }
}

// one wavefront per F1 entry (i, m): every b in A[m, :] adds w1 * w2 to the count of (i, b) in C2 (binary search in
// the sorted row), less the self-loop walk
__global__ __launch_bounds__(256) void trail2_count_kernel(CsrView f1, const u64* __restrict__ w1, CsrView a,
                                                          const u64* __restrict__ aw, CsrView c2,
                                                          const u32* __restrict__ src, u32 nnzf,
                                                          unsigned long long* __restrict__ counts) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    for (u32 e = wave; e < nnzf; e += nwaves) {
        u32 lo = 0, hi = f1.nrows - 1;                 // row of entry e
        while (lo < hi) {
            const u32 mid = (lo + hi + 1) >> 1;
            if (f1.rowptr[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const u32 i = lo, m = f1.colidx[e], s = src[i];
        const u64 wa = w1[e];
        u32 rb, re;
        row_range(a, m, rb, re);
        const u32 cb = c2.rowptr[i], ce = c2.rowptr[i + 1];
        for (u32 q = rb + lane; q < re; q += 64) {
            const u32 b = a.colidx[q];
            const u64 wb = aw ? aw[q] : 1ull;
            u64 add = wa * wb;
            if (m == s && b == s) add -= wa;           // a -> a -> a over the same edge: not a trail
            if (add == 0) continue;
            u32 l = cb, h = ce;
            while (l < h) {
                const u32 mid = (l + h) >> 1;
                if (c2.colidx[mid] < b) l = mid + 1; else h = mid;
            }
            atomicAdd(&counts[l], (unsigned long long)add);   // (i, b) is in C2 by construction
        }
    }
}

}  // namespace fgpu

using namespace fgpu;

// ---- (active_row, dest) columns built on the device (include/fgpu.h fgpu_expand_pairs) ------------------------------------
// rows the operator may keep: all of a free row, at most the one entry equal to the pinned destination of a pinned row
__global__ void pairs_len_kernel(const u32* __restrict__ rowptr, const u32* __restrict__ colidx, const u32* __restrict__ pin, u32 nsrc,
                                 u32* __restrict__ len, u32* __restrict__ pos) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nsrc) return;
    u32 l = 0, p = 0;
    if (i < nsrc) {
        const u32 b = rowptr[i], e = rowptr[i + 1];
        const u32 want = pin[i];
        if (want == 0xFFFFFFFFu) { l = e - b; p = b; }
        else if (want != 0xFFFFFFFEu) {                      // (0xFFFFFFFE: a pinned id beyond 32 bits — no vertex has it)
            u32 lo = b, hi = e;                              // destinations are ascending and unique per row
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (colidx[mid] < want) lo = mid + 1; else hi = mid;
            }
            if (lo < e && colidx[lo] == want) { l = 1; p = lo; }
        }
    }
    len[i] = l;
    pos[i] = p;
}
// a thread per OUTPUT entry: its row by a search of the (new) row pointers, its destination from the row's first kept entry
// (out_dest nullable: the 32-bit form of an unpinned batch ships the result's own column ids and only needs the row column)
template <typename RowT, typename DestT>
__global__ __launch_bounds__(256) void pairs_fill_kernel(const u32* __restrict__ newptr, const u32* __restrict__ pos,
                                                         const u32* __restrict__ colidx, u32 nsrc, u64 n,
                                                         RowT* __restrict__ out_row, DestT* __restrict__ out_dest) {
    for (u64 q = (u64)blockIdx.x * 256 + threadIdx.x; q < n; q += (u64)gridDim.x * 256) {
        u32 lo = 0, hi = nsrc - 1;                           // largest row with newptr[row] <= q
        while (lo < hi) {
            const u32 mid = (lo + hi + 1) >> 1;
            if (newptr[mid] <= q) lo = mid; else hi = mid - 1;
        }
        out_row[q] = (RowT)lo;
        if (out_dest) out_dest[q] = (DestT)colidx[pos[lo] + (u32)(q - newptr[lo])];
    }
}


// the last hop of an all-pinned batch from a SORTED-CSR frontier F: a wavefront per row i, a lane per entry u of F[i, :] — is
// dst[i] in m[u, :] / dm[u, :] / dp[u, :]?  (rows are ascending: binary search)
__global__ __launch_bounds__(256) void probe_csr_rows_kernel(CsrView f, CsrView m, CsrView dm, CsrView dp, const u32* __restrict__ dst,
                                                             u32 k, uint8_t* __restrict__ hit_m, uint8_t* __restrict__ hit_dm,
                                                             uint8_t* __restrict__ hit_dp) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    auto has = [](const CsrView& a, u32 u, u32 v) {
        if (!a.rowptr) return false;
        u32 b, e;
        row_range(a, u, b, e);
        while (b < e) {
            const u32 mid = (b + e) >> 1;
            if (a.colidx[mid] < v) b = mid + 1; else e = mid;
        }
        u32 b0, e0;
        row_range(a, u, b0, e0);
        return b < e0 && a.colidx[b] == v;
    };
    for (u32 i = wave; i < k; i += nwaves) {
        const u32 v = dst[i];
        if (v == 0xFFFFFFFFu) continue;
        const u32 fb = f.rowptr[i], fe = f.rowptr[i + 1];
        bool a = false, b = false, c = false;
        for (u32 q = fb + lane; q < fe; q += 64) {
            const u32 u = f.colidx[q];
            a = a || has(m, u, v);
            b = b || has(dm, u, v);
            c = c || has(dp, u, v);
        }
        if (__ballot(a) && lane == 0) hit_m[i] = 1;
        if (__ballot(b) && lane == 0) hit_dm[i] = 1;
        if (__ballot(c) && lane == 0) hit_dp[i] = 1;
    }
}

// nnz (+ checksum) of a chain that ended in CSR form; rowmap (nullable) = the call's row of every row of r, rowhash (nullable)
// = the hash of every row of r, which then stands in for cs_row_hash(rowmap[.])
static fgpu_info count_csr_result(fgpu_ctx* ctx, const fgpu_mat* r, const u32* rowmap, const u64* rowhash, u64* out_nnz,
                                  u64* checksum) {
    *out_nnz = r->nnz;
    if (!checksum) return FGPU_OK;
    *checksum = 0;
    if (!r->nnz) return FGPU_OK;
    DevBuf<u64> acc;
    FGPU_TRY(acc.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(acc.p, 0, sizeof(u64), ctx->stream()));
    if (r->nnz / r->nrows >= 1024 && r->nnz < 0xFFFFFFFFull) {
        u32 grid = cdiv(r->nnz, 256);
        if (grid > (u32)ctx->cus * 32) grid = ctx->cus * 32;
        FGPU_TRY(launch(checksum_entries_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(r),
                        (u32)r->nrows, (u32)r->nnz, (unsigned long long*)acc.p, rowmap, rowhash));
    } else {
        u32 grid = cdiv(r->nrows, 4);
        if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
        FGPU_TRY(launch(checksum_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(r),
                        (u32)r->nrows, (unsigned long long*)acc.p, rowmap, rowhash));
    }
    return read_u64(ctx, acc.p, checksum);
}

// ---- whole-frontier calls (SURVEY.md §7 "hard part 1", §8d) ---------------------------------------------------------------
// The reference hands CondTraverse at most 1024 rows per mxm (BATCH_SIZE, graph/src/runtime/batch.rs:81; the loop of
// cond_traverse.rs:452-751) — at that size a launch of this chip is latency, and half of a label scan's sources have no
// out-edge at all (an R-MAT graph: 525 of the first 1024 :P sources), so a 1024-source batch fills 64 of the 128 bytes of
// the row the count hop gathers per entry of A' and a missed gather costs a whole 128-byte line either way.
// fgpu_expand_count therefore takes ALL sources of a scan (10^5 - 10^6 rows) in one call:
//   1. the sources are filtered on the device: a row takes part when its source has an entry in m[0] or dp[0] (every other
//      row's result is empty whatever follows), and the live rows are compacted — (source id, row of the call) pairs;
//   2. the live rows are cut into PASSES of `expand_scan_rows` rows (1024: 16 words = one 128-byte line per vertex) — the
//      width is picked from the LIVE rows, not from the caller's batch size; over a clean hop 0 the sources of out-degree one
//      that share their target first become one row per class and power of two ("classes of degree-one sources" below), which
//      takes 5 % of the passes off an R-MAT label scan;
//   3. the passes are dealt to `expand_scan_lanes` lanes of the context (the calling thread + worker threads, each on its own
//      stream and pool: a chain makes ~10 host-side decisions per pass — product sizes, the CSR -> bit-form switch, the
//      counts — during which ITS stream idles), so one pass's launch-bound head and tail run under another's count hop;
//   4. rows keep their identity: bit i of a pass stands for row rowmap[i] of the call, which is what the checksum hashes.
// The sums are order-independent (64-bit wrap-around adds), so the result equals the 1024-row calls' sums bit for bit.
__global__ void scan_live_kernel(const u32* __restrict__ ids, u32 n, CsrView m0, CsrView dp0, u32 has_dp, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    u32 live = 0;
    if (i < n && ids[i] != 0xFFFFFFFFu) {
        u32 b, e;
        row_range(m0, ids[i], b, e);
        live = e > b;
        if (!live && has_dp) { row_range(dp0, ids[i], b, e); live = e > b; }
    }
    flag[i] = live;
}
__global__ void scan_compact_kernel(const u32* __restrict__ ids, const u32* __restrict__ flag, const u32* __restrict__ pos, u32 n,
                                    u32* __restrict__ lid, u32* __restrict__ lrow) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) { lid[pos[i]] = ids[i]; lrow[pos[i]] = i; }
}
// (lhash, nullable: the rows carry their hashes — a classed row list, below)
__global__ void scan_pass_kernel(const u32* __restrict__ lid, const u32* __restrict__ lrow, const u64* __restrict__ lhash, u32 first,
                                 u32 k, u32* __restrict__ rowptr, u32* __restrict__ colidx, u32* __restrict__ rowmap,
                                 u64* __restrict__ rowhash) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= k) rowptr[i] = i;
    if (i < k) {
        colidx[i] = lid[first + i];
        rowmap[i] = lrow[first + i];
        if (lhash) rowhash[i] = lhash[first + i];
    }
}

// ---- classes of degree-one sources ----------------------------------------------------------------------------------------
// nnz, flops and the checksum sum_(row, dest) cs_row_hash(row) * cs_dest_hash(dest) are 64-bit wrap-around sums that are LINEAR in
// the rows, and two sources with the same out-neighbour set over m[0] have identical result rows: they need one bit of a pass,
// whose hash is the sum of their row hashes and whose nnz and flops count twice.  A label scan of an R-MAT graph has such
// sources in bulk among those of out-degree ONE (28 % of the live rows of RMAT-22, on 3/4 as many targets; equal sets of two
// and more entries are one source in 10^5 there and are not looked for).  Over a clean hop 0 the live rows are therefore CLASSED
// by their single target:
//   * a class of m sources appears once in the pass group of scale 2^k for every set bit k < kmax of m, and m >> kmax times
//     in the top group; group 0 also holds the plain rows.  A pass holds rows of one scale, its nnz and flops are multiplied
//     by it on the host, and no kernel of the chain knows;
//   * the class's hash sum rides on the first of its rows in the lowest group it appears in, its other rows carry 0;
//   * kmax in [0, SCAN_KMAX] minimises the passes, sum_k ceil(rows_k / expand_scan_rows) (ties: the smaller; 0 = the live list
//     as it is), from one read-back of the classes' bit counts.
// The plan is deterministic: a class is named by its first member in live order, and every group lists its rows in that order.
// In group 0 the classes' rows stay BETWEEN the plain rows, where their first members were: its passes then hold the mix of
// light and heavy sources the chain's form decisions were measured on.  (Plain rows first and class rows after them made 22
// passes per RMAT-22 scan of degree-one sources only; ten of those stayed in CSR form up to the count hop and took its plain
// pull, 1.8 ms a launch, which cost 3/4 of what the saved passes gained: profiles/NOTES_scan_classes.md.)
constexpr u32 SCAN_KMAX = 5;
constexpr u32 SCAN_NOKEY = 0xFFFFFFFFu;

// key[i] = the single out-neighbour of live row i (SCAN_NOKEY: not of degree one); rep[t] = the first live row with key t
// (rep: ncols entries, all ones)
__global__ void scan_class_key_kernel(const u32* __restrict__ lid, u32 nlive, CsrView m0, u32 ncols, u32* __restrict__ key,
                                      u32* __restrict__ rep) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlive) return;
    u32 b, e;
    row_range(m0, lid[i], b, e);
    u32 t = SCAN_NOKEY;
    if (e - b == 1 && m0.colidx[b] < ncols) {
        t = m0.colidx[b];
        atomicMin(&rep[t], i);
    }
    key[i] = t;
}
// members and hash sum of every class, at its first member (cnt and hsum zeroed, one entry per live row)
__global__ void scan_class_sum_kernel(const u32* __restrict__ lrow, const u32* __restrict__ key, const u32* __restrict__ rep, u32 nlive,
                                      u32* __restrict__ cnt, unsigned long long* __restrict__ hsum) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlive || key[i] == SCAN_NOKEY) return;
    const u32 r = rep[key[i]];
    atomicAdd(&cnt[r], 1u);
    atomicAdd(&hsum[r], (unsigned long long)cs_row_hash(lrow[i]));
}
// stats[k] = classes with bit k of m set, stats[SCAN_KMAX + 1 + k] = sum of m >> k, k = 0 .. SCAN_KMAX
// (a grid-stride loop and a sum per workgroup: twelve atomics per wavefront of a launch over all live rows took 92 us on the
// twelve words)
__global__ __launch_bounds__(256) void scan_class_stats_kernel(const u32* __restrict__ cnt, u32 nlive, u32* __restrict__ stats) {
    __shared__ u32 s_sum[2 * (SCAN_KMAX + 1)];
    if (threadIdx.x < 2 * (SCAN_KMAX + 1)) s_sum[threadIdx.x] = 0;
    __syncthreads();
    u32 a[SCAN_KMAX + 1] = {}, s[SCAN_KMAX + 1] = {};
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < nlive; i += gridDim.x * 256) {
        const u32 m = cnt[i];                       // (0 everywhere but at a class's first member)
#pragma unroll
        for (u32 k = 0; k <= SCAN_KMAX; ++k) { a[k] += (m >> k) & 1u; s[k] += m >> k; }
    }
#pragma unroll
    for (u32 k = 0; k <= SCAN_KMAX; ++k) {
        u32 x = a[k], y = s[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { x += __shfl_xor(x, d, 64); y += __shfl_xor(y, d, 64); }
        if (lane_id() == 0 && x) atomicAdd(&s_sum[k], x);
        if (lane_id() == 0 && y) atomicAdd(&s_sum[SCAN_KMAX + 1 + k], y);
    }
    __syncthreads();
    if (threadIdx.x < 2 * (SCAN_KMAX + 1) && s_sum[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_sum[threadIdx.x]);
}
// rows live row i contributes to group k of the row list (kmax >= 1; m = cnt[i]: 0 but at a class's first member)
__device__ __forceinline__ u32 scan_class_rows_of(u32 k, u32 key, u32 m, u32 kmax) {
    if (key == SCAN_NOKEY) return k == 0;
    return k < kmax ? (m >> k) & 1u : m >> kmax;
}
__global__ void scan_class_rows_kernel(const u32* __restrict__ key, const u32* __restrict__ cnt, u32 nlive, u32 kmax, u32* __restrict__ c) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) c[(u64)(kmax + 1) * nlive] = 0;
    if (i >= nlive) return;
    for (u32 k = 0; k <= kmax; ++k) c[(u64)k * nlive + i] = scan_class_rows_of(k, key[i], cnt[i], kmax);
}
// the row list: (source id, row of the call, row hash) at the scanned positions, nrows of them
__global__ void scan_class_fill_kernel(const u32* __restrict__ lid, const u32* __restrict__ lrow, const u32* __restrict__ key,
                                       const u32* __restrict__ cnt, const u64* __restrict__ hsum, const u32* __restrict__ pos, u32 nlive,
                                       u32 kmax, u32 nrows, u32* __restrict__ rid, u32* __restrict__ rrow, u64* __restrict__ rhash) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 k = blockIdx.y;
    if (i >= nlive) return;
    const u32 m = cnt[i];
    const u32 n = scan_class_rows_of(k, key[i], m, kmax);
    if (!n) return;
    u64 h;
    if (key[i] == SCAN_NOKEY) h = cs_row_hash(lrow[i]);
    else {
        const u32 low = (u32)__ffs(m) - 1;                       // the lowest group of the class: its lowest set bit, or the top group
        h = (k == (low < kmax ? low : kmax)) ? hsum[i] : 0ull;
    }
    const u32 p = pos[(u64)k * nlive + i];
    for (u32 q = 0; q < n && p + q < nrows; ++q) {
        rid[p + q] = lid[i];
        rrow[p + q] = lrow[i];
        rhash[p + q] = q ? 0ull : h;
    }
}

// ---- strong sources first -------------------------------------------------------------------------------------------------
// The count hop of a 3-hop scan skips the out-rows of its matrix's top hub h in a pass whose EVERY source reaches h in exactly
// two hops (bitexpand.hip bp_hub_rows: row h of the state is then all ones).  86 % of the live sources of an RMAT-22 label scan
// do, but a pass of 1024 sources in id order never holds such sources only.  Over clean layers the live list is therefore
// stable-partitioned: the sources with an out-neighbour that has an edge to h ("strong") first, the others after them.  Members
// of a degree-one class share their target, hence their strength, and the classing below works on the reordered list as it is.
// The order is a heuristic and nothing else: the hop tests the state it is given, whatever order the sources came in.
// weak[i] = 0 when live row i is strong (weak[nlive] = 0: the scan leaves the number of weak rows there)
__global__ void scan_strong_kernel(const u32* __restrict__ lid, u32 nlive, CsrView m0, const u64* __restrict__ in_h, u32 nbits,
                                   u32* __restrict__ weak) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nlive) return;
    u32 w = 0;
    if (i < nlive) {
        u32 b, e;
        row_range(m0, lid[i], b, e);
        w = 1;
        for (u32 q = b; q < e && w; ++q) {
            const u32 t = m0.colidx[q];
            if (t < nbits && ((in_h[t >> 6] >> (t & 63u)) & 1ull)) w = 0;
        }
    }
    weak[i] = w;
}
// With a second reduced plan (bitpart.hip bp_xplan_hub_set_build) the strong sources come in two tiers: tier A reaches EVERY hub of
// the set H in exactly two hops — its passes run under the second plan — tier B reaches the top hub but not all of H.  The list
// becomes A, B, weak, each in its old order.  mask[t] = bit i: t has an edge to H[i]; `all` = the nh low bits.
// mid[i] = 1 when live row i is of tier B, weak[i] = 1 when it is weak (both 0 at i = nlive, for the scans' totals)
__global__ void scan_tier_kernel(const u32* __restrict__ lid, u32 nlive, CsrView m0, const u32* __restrict__ mask, u32 nbits, u32 all,
                                 u32* __restrict__ mid, u32* __restrict__ weak) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nlive) return;
    u32 got = all;
    if (i < nlive) {
        u32 b, e;
        row_range(m0, lid[i], b, e);
        got = 0;
        for (u32 q = b; q < e && got != all; ++q) {
            const u32 t = m0.colidx[q];
            if (t < nbits) got |= mask[t] & all;
        }
    }
    mid[i] = (got & 1u) && got != all ? 1u : 0u;
    weak[i] = (got & 1u) ? 0u : 1u;
}
// mid / mpos = nullptr: two tiers (strong, weak)
__global__ void scan_strong_move_kernel(const u32* __restrict__ lid, const u32* __restrict__ lrow, const u32* __restrict__ weak,
                                        const u32* __restrict__ wpos, const u32* __restrict__ mid, const u32* __restrict__ mpos,
                                        u32 nlive, u32* __restrict__ olid, u32* __restrict__ olrow) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlive) return;
    const u32 nweak = wpos[nlive], nmid = mid ? mpos[nlive] : 0u, mbefore = mid ? mpos[i] : 0u;
    const u32 p = weak[i]               ? nlive - nweak + wpos[i]
                  : (mid && mid[i])     ? nlive - nweak - nmid + mbefore
                                        : i - wpos[i] - mbefore;
    olid[p] = lid[i];
    olrow[p] = lrow[i];
}
// reorders (lid, lrow) strong-first when the call is a clean 3-hop chain whose last two hops run over one snapshot that has a
// reduced plan for the count hop — tier A, tier B, weak when it has two; leaves them alone otherwise
static fgpu_info scan_strong_first(fgpu_ctx* ctx, const Layers& L, DevBuf<u32>& lid, DevBuf<u32>& lrow, u32 nlive, u32 pass_rows) {
    if (L.nhops != 3 || L.m[1] != L.m[2] || L.m[0]->ncols != L.m[1]->nrows) return FGPU_OK;
    for (int h = 0; h < 3; ++h)
        if ((L.dp_at(h) && L.dp_at(h)->nnz) || (L.dm_at(h) && L.dm_at(h)->nnz)) return FGPU_OK;
    const u64* in_h = nullptr;
    const u32* mask = nullptr;
    u32 nh = 0;
    FGPU_TRY(bp_count_hub_in(ctx, L.m[2], pass_rows, &in_h, &mask, &nh));
    if (!in_h) return FGPU_OK;
    ProfScope ps(ctx, "scan strong first", 0);
    DevBuf<u32> weak, wpos, mid, mpos, olid, olrow;
    FGPU_TRY(weak.alloc(ctx, (size_t)nlive + 1));
    FGPU_TRY(wpos.alloc(ctx, (size_t)nlive + 1));
    FGPU_TRY(olid.alloc(ctx, nlive));
    FGPU_TRY(olrow.alloc(ctx, nlive));
    if (mask && nh >= 2) {
        FGPU_TRY(mid.alloc(ctx, (size_t)nlive + 1));
        FGPU_TRY(mpos.alloc(ctx, (size_t)nlive + 1));
        const u32 all = nh >= 32 ? 0xFFFFFFFFu : (1u << nh) - 1u;
        FGPU_TRY(launch(scan_tier_kernel, dim3(cdiv((u64)nlive + 1, 256)), dim3(256), 0, ctx->stream(), (const u32*)lid.p, nlive,
                        view_of(L.m[0]), mask, (u32)L.m[1]->nrows, all, mid.p, weak.p));
        FGPU_TRY(scan_u32(ctx, mid.p, mpos.p, (u64)nlive + 1, nullptr));
    } else {
        FGPU_TRY(launch(scan_strong_kernel, dim3(cdiv((u64)nlive + 1, 256)), dim3(256), 0, ctx->stream(), (const u32*)lid.p, nlive,
                        view_of(L.m[0]), in_h, (u32)L.m[1]->nrows, weak.p));
    }
    FGPU_TRY(scan_u32(ctx, weak.p, wpos.p, (u64)nlive + 1, nullptr));
    FGPU_TRY(launch(scan_strong_move_kernel, dim3(cdiv(nlive, 256)), dim3(256), 0, ctx->stream(), (const u32*)lid.p, (const u32*)lrow.p,
                    (const u32*)weak.p, (const u32*)wpos.p, (const u32*)mid.p, (const u32*)mpos.p, nlive, olid.p, olrow.p));
    lid = std::move(olid);
    lrow = std::move(olrow);
    return FGPU_OK;
}

struct ScanPass { u32 first, rows, scale; };

// the passes of `groups` consecutive row groups (rows[g] rows at scale 2^g): `pass_rows` rows each, never across a group boundary
static void scan_cut_passes(const u32* rows, u32 groups, u32 pass_rows, std::vector<ScanPass>& out) {
    u32 first = 0;
    for (u32 g = 0; g < groups; ++g) {
        for (u32 o = 0; o < rows[g]; o += pass_rows) out.push_back({first + o, std::min(pass_rows, rows[g] - o), 1u << g});
        first += rows[g];
    }
}

// the classed row list of a whole-frontier call over a clean hop 0 (above); kmax = 0 on return: the live list stays as it is
struct ScanClasses {
    DevBuf<u32> rid, rrow;
    DevBuf<u64> rhash;
    u32 kmax = 0;
    u32 rows[SCAN_KMAX + 1] = {};
};
static fgpu_info scan_build_classes(fgpu_ctx* ctx, const fgpu_mat* m0, const u32* lid, const u32* lrow, u32 nlive, u32 pass_rows,
                                    ScanClasses& sc) {
    ProfScope ps(ctx, "scan classes", 0);
    DevBuf<u32> key, rep, cnt, stats;
    DevBuf<u64> hsum;
    const u32 grid = cdiv(nlive, 256);
    FGPU_TRY(key.alloc(ctx, nlive));
    FGPU_TRY(cnt.alloc(ctx, nlive));
    FGPU_TRY(hsum.alloc(ctx, nlive));
    FGPU_TRY(rep.alloc(ctx, m0->ncols));
    FGPU_TRY(stats.alloc(ctx, 2 * (SCAN_KMAX + 1)));
    FGPU_HIP(hipMemsetAsync(rep.p, 0xFF, (size_t)m0->ncols * sizeof(u32), ctx->stream()));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, (size_t)nlive * sizeof(u32), ctx->stream()));
    FGPU_HIP(hipMemsetAsync(hsum.p, 0, (size_t)nlive * sizeof(u64), ctx->stream()));
    FGPU_HIP(hipMemsetAsync(stats.p, 0, 2 * (SCAN_KMAX + 1) * sizeof(u32), ctx->stream()));
    FGPU_TRY(launch(scan_class_key_kernel, dim3(grid), dim3(256), 0, ctx->stream(), lid, nlive, view_of(m0), (u32)m0->ncols, key.p,
                    rep.p));
    FGPU_TRY(launch(scan_class_sum_kernel, dim3(grid), dim3(256), 0, ctx->stream(), lrow, (const u32*)key.p, (const u32*)rep.p, nlive,
                    cnt.p, (unsigned long long*)hsum.p));
    FGPU_TRY(launch(scan_class_stats_kernel, dim3(std::min(grid, 32u)), dim3(256), 0, ctx->stream(), (const u32*)cnt.p, nlive, stats.p));
    u32 st[2 * (SCAN_KMAX + 1)];
    FGPU_TRY(read_words(ctx, stats.p, 2 * (SCAN_KMAX + 1), st));
    const u32* bits = st;                       // classes with bit k of m set
    const u32* top = st + SCAN_KMAX + 1;        // sum of m >> k
    const u32 nplain = nlive - top[0];
    u32 best = 0;
    for (u32 kmax = 0; kmax <= SCAN_KMAX; ++kmax) {
        u32 passes = 0;
        for (u32 k = 0; k <= kmax; ++k) passes += cdiv((k ? 0u : nplain) + (k < kmax ? bits[k] : top[k]), pass_rows);
        if (kmax == 0 || passes < best) { best = passes; sc.kmax = kmax; }
    }
    if (sc.kmax == 0) return FGPU_OK;
    const u32 kmax = sc.kmax;
    u32 nrows = 0;
    for (u32 k = 0; k <= kmax; ++k) nrows += sc.rows[k] = (k ? 0u : nplain) + (k < kmax ? bits[k] : top[k]);
    DevBuf<u32> c, pos;
    const u64 nc = (u64)(kmax + 1) * nlive + 1;
    FGPU_TRY(c.alloc(ctx, nc));
    FGPU_TRY(pos.alloc(ctx, nc));
    FGPU_TRY(sc.rid.alloc(ctx, nrows));
    FGPU_TRY(sc.rrow.alloc(ctx, nrows));
    FGPU_TRY(sc.rhash.alloc(ctx, nrows));
    FGPU_TRY(launch(scan_class_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream(), (const u32*)key.p, (const u32*)cnt.p, nlive, kmax, c.p));
    FGPU_TRY(scan_u32(ctx, c.p, pos.p, nc, nullptr));
    FGPU_TRY(launch(scan_class_fill_kernel, dim3(grid, kmax + 1), dim3(256), 0, ctx->stream(), lid, lrow, (const u32*)key.p,
                    (const u32*)cnt.p, (const u64*)hsum.p, (const u32*)pos.p, nlive, kmax, nrows, sc.rid.p, sc.rrow.p, sc.rhash.p));
    return FGPU_OK;
}

struct ScanJob {
    fgpu_ctx* ctx;
    const u32 *lid, *lrow;               // the row list: source id and row of the call ...
    const u64* lhash = nullptr;          // ... and, for a classed list, the row's hash
    std::vector<ScanPass> passes;
    u32 npasses;
    Layers L;
    const uint64_t* label;
    bool want_cs, want_flops;
    std::atomic<u32> next{0};
    std::atomic<bool> failed{false};
    std::mutex mu;                       // the sums and the first error
    u64 nnz = 0, cs = 0, flops = 0;
    fgpu_info err = FGPU_OK;
    std::string msg;
};

static fgpu_info scan_one_pass(ScanJob& j, u32 p, u64* nnz, u64* cs, u64* fl) {
    fgpu_ctx* ctx = j.ctx;
    const ScanPass& ps = j.passes[p];
    const u32 first = ps.first, k = ps.rows;
    const u64* lhash = j.want_cs ? j.lhash : nullptr;      // (only the checksum reads the hashes)
    DevBuf<u32> rm;
    DevBuf<u64> rh;
    ChainSources pre;
    FGPU_TRY(rm.alloc(ctx, k));
    if (lhash) FGPU_TRY(rh.alloc(ctx, k));
    FGPU_TRY(mat_alloc(ctx, &pre.f.m, k, j.L.m[0]->nrows, k, false, 0, false));
    FGPU_TRY(launch(scan_pass_kernel, dim3(cdiv((u64)k + 1, 256)), dim3(256), 0, ctx->stream(), j.lid, j.lrow, lhash, first, k,
                    pre.f->rowptr, pre.f->colidx, rm.p, rh.p));
    pre.rowmap = &rm;
    if (lhash) pre.rowhash = &rh;
    *fl = 0;
    const ChainRequest rq{nullptr, k, j.L, j.label, j.want_flops ? fl : nullptr, j.want_cs ? ChainEnd::CountSum : ChainEnd::Count, &pre};
    ChainResult r;
    FGPU_TRY(expand_device(ctx, rq, r));
    if (r.kind == ChainResult::Counts) { *nnz = r.nnz; *cs = r.checksum; }
    else FGPU_TRY(count_csr_result(ctx, r.mat.get(), rm.p, rh.p, nnz, j.want_cs ? cs : nullptr));
    // every row of the pass stands for `scale` rows of the call with the same result row (the checksum's hashes say so already)
    *nnz *= ps.scale;
    *fl *= ps.scale;
    return FGPU_OK;
}

static void scan_worker(ScanJob* j) {
    u64 nnz = 0, cs = 0, flops = 0;
    fgpu_info err = FGPU_OK;
    for (;;) {
        if (j->failed.load(std::memory_order_relaxed)) break;
        const u32 p = j->next.fetch_add(1, std::memory_order_relaxed);
        if (p >= j->npasses) break;
        u64 a = 0, b = 0, c = 0;
        err = scan_one_pass(*j, p, &a, &b, &c);
        if (err != FGPU_OK) {
            // the pass may have left kernels queued on this lane's stream that read lid / lrow, which the caller frees once
            // the workers are joined: wait for them (whatever the wait returns, the first error is the one reported)
            (void)hipStreamSynchronize(j->ctx->stream());
            j->failed.store(true);
            break;
        }
        nnz += a; cs += b; flops += c;
    }
    // (after a successful pass the lane's stream has nothing pending: every pass ends with the read-back of its sums; after a
    // failed one it was drained above)
    std::lock_guard<std::mutex> g(j->mu);
    j->nnz += nnz; j->cs += cs; j->flops += flops;
    if (err != FGPU_OK && j->err == FGPU_OK) { j->err = err; j->msg = get_error(); }
}

static fgpu_info expand_count_scan(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const Layers& L,
                                   const uint64_t* dst_label_bitmap, uint64_t* out_nnz, uint64_t* checksum, uint64_t* flops) {
    FGPU_TRY(check_hops(L, nsrc));
    const fgpu_mat* const* m = L.m;
    const u64 ncols0 = m[0]->nrows;
    const u32 n = (u32)nsrc;
    std::vector<u32> ids(n);
    for (u32 i = 0; i < n; ++i) {
        if (src_ids[i] == UINT64_MAX) { ids[i] = 0xFFFFFFFFu; continue; }
        FGPU_REQUIRE(src_ids[i] < ncols0, FGPU_OUT_OF_BOUNDS, "expand: source %u = %llu >= %llu", i,
                     (unsigned long long)src_ids[i], (unsigned long long)ncols0);
        ids[i] = (u32)src_ids[i];
    }
    DevBuf<u32> dids, flag, pos, lid, lrow;
    FGPU_TRY(dids.alloc(ctx, n));
    FGPU_TRY(flag.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(pos.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(ctx->h2d(dids.p, ids.data(), (size_t)n * sizeof(u32)));
    const fgpu_mat* dp0 = L.dp_at(0) && L.dp_at(0)->nnz ? L.dp_at(0) : nullptr;
    FGPU_TRY(launch(scan_live_kernel, dim3(cdiv((u64)n + 1, 256)), dim3(256), 0, ctx->stream(), (const u32*)dids.p, n, view_of(m[0]),
                    dp0 ? view_of(dp0) : view_of(m[0]), dp0 ? 1u : 0u, flag.p));
    FGPU_TRY(scan_u32(ctx, flag.p, pos.p, (u64)n + 1, nullptr));
    u32 nlive = 0;
    FGPU_TRY(read_u32(ctx, pos.p + n, &nlive));
    *out_nnz = 0;
    if (checksum) *checksum = 0;
    ctx->scan_last_live.store(nlive, std::memory_order_relaxed);
    ctx->scan_last_passes.store(0, std::memory_order_relaxed);
    if (nlive == 0) return FGPU_OK;
    FGPU_TRY(lid.alloc(ctx, nlive));
    FGPU_TRY(lrow.alloc(ctx, nlive));
    FGPU_TRY(launch(scan_compact_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream(), (const u32*)dids.p, (const u32*)flag.p,
                    (const u32*)pos.p, n, lid.p, lrow.p));
    const u32 pass_rows = (u32)ctx->opt.expand_scan_rows;
    // (a call of one pass has nothing to order)
    if (nlive > pass_rows) FGPU_TRY(scan_strong_first(ctx, L, lid, lrow, nlive, pass_rows));
    // over a clean hop 0 the degree-one sources are classed by their target (scan_build_classes); over a dirty one a row of m[0]
    // is not the source's out-neighbour set, and every row stays a row of scale 1
    const fgpu_mat* dm0 = L.dm_at(0) && L.dm_at(0)->nnz ? L.dm_at(0) : nullptr;
    ScanClasses sc;
    if (!dp0 && !dm0) FGPU_TRY(scan_build_classes(ctx, m[0], lid.p, lrow.p, nlive, pass_rows, sc));
    FGPU_HIP(hipStreamSynchronize(ctx->stream()));           // the other lanes read the row list
    ScanJob j;
    j.ctx = ctx;
    if (sc.kmax) {
        j.lid = sc.rid.p; j.lrow = sc.rrow.p; j.lhash = sc.rhash.p;
        scan_cut_passes(sc.rows, sc.kmax + 1, pass_rows, j.passes);
    } else {
        j.lid = lid.p; j.lrow = lrow.p;
        scan_cut_passes(&nlive, 1, pass_rows, j.passes);
    }
    j.npasses = (u32)j.passes.size();
    j.L = L; j.label = dst_label_bitmap;
    j.want_cs = checksum != nullptr; j.want_flops = flops != nullptr;
    ctx->scan_last_passes.store(j.npasses, std::memory_order_relaxed);
    u32 lanes = (u32)ctx->opt.expand_scan_lanes;
    if (lanes > j.npasses) lanes = j.npasses;
    if (lanes < 1) lanes = 1;
    std::vector<std::thread> th;
    th.reserve(lanes);
    ctx->scan_active.fetch_add((int)lanes, std::memory_order_relaxed);
    for (u32 t = 1; t < lanes; ++t) {
        try { th.emplace_back(scan_worker, &j); } catch (...) { break; }   // (fewer lanes: the passes are pulled, not assigned)
    }
    scan_worker(&j);
    for (auto& t : th) t.join();
    ctx->scan_active.fetch_sub((int)lanes, std::memory_order_relaxed);
    if (j.err != FGPU_OK) { set_error("%s", j.msg.c_str()); return j.err; }
    *out_nnz = j.nnz;
    if (checksum) *checksum = j.cs;
    if (flops) *flops = j.flops;
    return FGPU_OK;
}

extern "C" {

static fgpu_info mxm_impl(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* b) {
    FGPU_REQUIRE(ctx && c && f && b, FGPU_NULL_POINTER, "fgpu_mxm: NULL argument");
    return mxm_device(ctx, c, f, b, nullptr);
}

static fgpu_info delta_lmxm_impl(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* m, const fgpu_mat* dp,
                          const fgpu_mat* dm) {
    FGPU_REQUIRE(ctx && c && f && m, FGPU_NULL_POINTER, "fgpu_delta_lmxm: NULL argument");
    FGPU_REQUIRE(!dp || (dp->nrows == m->nrows && dp->ncols == m->ncols), FGPU_DIM_MISMATCH,
                 "fgpu_delta_lmxm: dp dims differ from m");
    FGPU_REQUIRE(!dm || (dm->nrows == m->nrows && dm->ncols == m->ncols), FGPU_DIM_MISMATCH,
                 "fgpu_delta_lmxm: dm dims differ from m");
    return delta_lmxm_device(ctx, c, f, m, dp, dm, nullptr);
}

fgpu_info fgpu_expand(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                      const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                      const uint64_t* dst_label_bitmap, uint64_t** out_rowptr, uint64_t** out_dest,
                      uint64_t* out_nnz, uint64_t* flops) {
    FGPU_REQUIRE(ctx && out_rowptr && out_dest && out_nnz, FGPU_NULL_POINTER, "fgpu_expand: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand: NULL src_ids");
    if (flops) *flops = 0;
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, ChainEnd::Csr}, res));
    uint64_t *vals = nullptr;
    return fgpu_mat_export_csr(ctx, res.mat.get(), out_rowptr, out_dest, &vals, out_nnz);
}

static fgpu_info expand_pairs_impl(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                                   const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                                   const uint64_t* pinned_dest, int row_bits, int dest_bits, void** out_row, void** out_dest, uint64_t* out_n,
                                   uint64_t* flops) {
    FGPU_REQUIRE(ctx && out_row && out_dest && out_n, FGPU_NULL_POINTER, "fgpu_expand_pairs: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_pairs: NULL src_ids");
    FGPU_REQUIRE(row_bits == 16 || row_bits == 32, FGPU_INVALID, "fgpu_expand_pairs: row_bits must be 16 or 32");
    FGPU_REQUIRE(row_bits == 32 || nsrc <= 65536, FGPU_INVALID, "fgpu_expand_pairs: %llu source rows do not fit 16-bit row indices",
                 (unsigned long long)nsrc);
    *out_row = nullptr; *out_dest = nullptr; *out_n = 0;
    if (flops) *flops = 0;
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, ChainEnd::Csr}, res));
    const fgpu_mat* r = res.mat.get();
    if (nsrc == 0 || r->nnz == 0) return FGPU_OK;
    // (the kernels below index the result's row pointers densely, nsrc + 1 of them)
    FGPU_REQUIRE(!r->is_hyper() && r->nrows == nsrc, FGPU_INVALID, "fgpu_expand_pairs: the chain's result is not a dense-row CSR of %llu rows",
                 (unsigned long long)nsrc);
    hipStream_t st = ctx->stream();
    const u32 k = (u32)nsrc;
    DevBuf<u32> pin, len, pos, newptr, total;
    FGPU_TRY(pin.alloc(ctx, k + 1));
    FGPU_TRY(len.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(pos.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(newptr.alloc(ctx, (size_t)k + 1));
    FGPU_TRY(total.alloc(ctx, 1));
    u64 n = r->nnz;
    const u32* rowptr = r->rowptr;                           // (no pinned row: the result's own row pointers and entries)
    const u32* first = r->rowptr;
    if (pinned_dest) {
        std::vector<u32> hp(k);
        bool any = false;
        for (u32 i = 0; i < k; ++i) {
            hp[i] = pinned_dest[i] == ~0ull ? 0xFFFFFFFFu : pinned_dest[i] >= 0xFFFFFFFEull ? 0xFFFFFFFEu : (u32)pinned_dest[i];
            any = any || hp[i] != 0xFFFFFFFFu;
        }
        if (any) {
            FGPU_TRY(ctx->h2d(pin.p, hp.data(), (size_t)k * sizeof(u32)));
            FGPU_TRY(launch(pairs_len_kernel, dim3(cdiv((u64)k + 1, 256)), dim3(256), 0, st, (const u32*)r->rowptr, (const u32*)r->colidx,
                            (const u32*)pin.p, k, len.p, pos.p));
            FGPU_TRY(scan_u32(ctx, len.p, newptr.p, (u64)k + 1, total.p));
            u32 t = 0;
            FGPU_TRY(read_u32(ctx, total.p, &t));
            n = t;
            rowptr = newptr.p;
            first = pos.p;
        }
    }
    if (n == 0) return FGPU_OK;
    const size_t rb = row_bits / 8, db = dest_bits / 8;
    // the 32-bit form of a batch without pinned rows: the destination column IS the result's column-id array
    const bool dest_is_colidx = dest_bits == 32 && rowptr == r->rowptr;
    DevBuf<uint8_t> ddest, drow;
    if (!dest_is_colidx) FGPU_TRY(ddest.alloc(ctx, n * db));
    FGPU_TRY(drow.alloc(ctx, n * rb));
    {
        ProfScope ps(ctx, "pairs_fill_kernel", n * (4 + (dest_is_colidx ? 0 : db) + rb));
        u32 grid = cdiv(n, 256 * 4);
        if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
        if (!grid) grid = 1;
        FGPU_TRY(pick(row_bits == 16, [&](auto r16) {
            return pick(dest_bits == 64, [&](auto d64) {
                using RT = std::conditional_t<decltype(r16)::value, uint16_t, u32>;
                using DT = std::conditional_t<decltype(d64)::value, u64, u32>;
                return launch(pairs_fill_kernel<RT, DT>, dim3(grid), dim3(256), 0, st, rowptr, first, (const u32*)r->colidx, k, n,
                              (RT*)drow.p, (DT*)ddest.p);
            });
        }));
    }
    ResultBuf hrow, hdest;
    FGPU_REQUIRE(hrow.alloc(ctx, n * rb) && hdest.alloc(ctx, n * db), FGPU_OOM, "fgpu_expand_pairs: host allocation failed");
    FGPU_TRY(ctx->d2h(hdest.p, dest_is_colidx ? (const void*)r->colidx : (const void*)ddest.p, n * db));
    FGPU_TRY(ctx->d2h(hrow.p, drow.p, n * rb));
    *out_row = hrow.release();
    *out_dest = hdest.release();
    *out_n = n;
    return FGPU_OK;
}

fgpu_info fgpu_expand_pairs(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                            const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                            const uint64_t* pinned_dest, int row_bits, void** out_row, uint64_t** out_dest, uint64_t* out_n,
                            uint64_t* flops) {
    return expand_pairs_impl(ctx, src_ids, nsrc, m, dp, dm, nhops, dst_label_bitmap, pinned_dest, row_bits, 64, out_row, (void**)out_dest,
                             out_n, flops);
}

fgpu_info fgpu_expand_pairs32(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                              const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                              const uint64_t* pinned_dest, int row_bits, void** out_row, uint32_t** out_dest, uint64_t* out_n,
                              uint64_t* flops) {
    return expand_pairs_impl(ctx, src_ids, nsrc, m, dp, dm, nhops, dst_label_bitmap, pinned_dest, row_bits, 32, out_row, (void**)out_dest,
                             out_n, flops);
}

fgpu_info fgpu_expand_probe(fgpu_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, uint64_t nsrc, const fgpu_mat* const* m,
                            const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap,
                            uint8_t* present, uint64_t* flops) {
    FGPU_REQUIRE(ctx && present && (nsrc == 0 || (src_ids && dst_ids)), FGPU_NULL_POINTER, "fgpu_expand_probe: NULL argument");
    if (flops) *flops = 0;
    const Layers L{m, dp, dm, nhops};
    FGPU_TRY(check_hops(L, nsrc));
    if (nsrc == 0) return FGPU_OK;
    const u32 k = (u32)nsrc;
    memset(present, 0, k);
    const fgpu_mat *ml = m[nhops - 1], *dpl = L.dp_at(nhops - 1), *dml = L.dm_at(nhops - 1);
    // the chain up to the last hop: a sorted-CSR frontier (f), or the bit state it ended in (bs)
    ChainResult res;
    if (nhops == 1) FGPU_TRY(upload_sources(ctx, &res.mat.m, src_ids, nsrc, m[0]->nrows));
    else FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops - 1}, nullptr, flops, ChainEnd::Bits}, res));
    const fgpu_mat* f = res.kind == ChainResult::Bits ? nullptr : res.mat.get();
    BitState& bs = res.bits;
    // destinations (a vertex the last matrix does not have, or one the label filter drops: no match), the bit of every row
    const u64 ncols = ml->ncols;
    std::vector<u32> hdst(k), hbit(k), order(k), sdst(k), srow(k);
    std::vector<u32> rank;
    if (!f && bs.nsrc_full) {
        rank.resize((size_t)bs.nsrc_full + 1);
        FGPU_TRY(ctx->d2h(rank.data(), bs.rowrank.p, rank.size() * sizeof(u32)));
    }
    for (u32 i = 0; i < k; ++i) {
        u64 v = dst_ids[i];
        if (v >= ncols || src_ids[i] == UINT64_MAX) v = ~0ull;
        else if (dst_label_bitmap && !((dst_label_bitmap[v >> 6] >> (v & 63)) & 1ull)) v = ~0ull;
        hdst[i] = v == ~0ull ? 0xFFFFFFFFu : (u32)v;
        if (rank.empty()) hbit[i] = i;
        else hbit[i] = rank[i + 1] > rank[i] ? rank[i] : 0xFFFFFFFFu;   // (a source row dropped before the chain went to bits is empty)
        order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return hdst[a] < hdst[b] || (hdst[a] == hdst[b] && a < b); });
    for (u32 p = 0; p < k; ++p) { sdst[p] = hdst[order[p]]; srow[p] = order[p]; }
    DevBuf<u32> d_dst, d_bit, d_sdst, d_srow;
    DevBuf<uint8_t> hits;
    FGPU_TRY(d_dst.alloc(ctx, k)); FGPU_TRY(d_bit.alloc(ctx, k)); FGPU_TRY(d_sdst.alloc(ctx, k)); FGPU_TRY(d_srow.alloc(ctx, k));
    FGPU_TRY(hits.alloc(ctx, (size_t)3 * k));
    FGPU_TRY(ctx->h2d(d_dst.p, hdst.data(), (size_t)k * 4));
    FGPU_TRY(ctx->h2d(d_bit.p, hbit.data(), (size_t)k * 4));
    FGPU_TRY(ctx->h2d(d_sdst.p, sdst.data(), (size_t)k * 4));
    FGPU_TRY(ctx->h2d(d_srow.p, srow.data(), (size_t)k * 4));
    FGPU_HIP(hipMemsetAsync(hits.p, 0, (size_t)3 * k, ctx->stream()));
    if (f) {
        if (f->nnz) {
            CsrView none;
            none.rowptr = nullptr; none.colidx = nullptr; none.hrows = nullptr; none.nvec = 0; none.nrows = 0;
            u32 grid = cdiv(k, 4);
            if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
            FGPU_TRY(launch(probe_csr_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(f), view_of(ml),
                            (dml && dml->nnz) ? view_of(dml) : none, (dpl && dpl->nnz) ? view_of(dpl) : none, (const u32*)d_dst.p, k,
                            hits.p, hits.p + k, hits.p + 2 * (size_t)k));
        }
    } else {
        FGPU_TRY(bp_probe_rows(ctx, bs, ml, dpl, dml, d_dst.p, d_bit.p, d_sdst.p, d_srow.p, k, hits.p, hits.p + k, hits.p + 2 * (size_t)k));
    }
    std::vector<uint8_t> h((size_t)3 * k);
    FGPU_TRY(ctx->d2h(h.data(), hits.p, (size_t)3 * k));
    if (!f) bp_finish(ctx, bs);
    // (F·m)<not (F·dm)> U (F·dp), one entry of it: the row-level mask of Matrix::delta_lmxm (matrix.rs:1343-1361)
    for (u32 i = 0; i < k; ++i) present[i] = ((h[i] && !h[k + i]) || h[2 * (size_t)k + i]) ? 1 : 0;
    return FGPU_OK;
}

// The pattern predicate (SemiApply / AntiSemiApply over a CondTraverse with an unbound destination, semi_apply.rs:85-106): bit i
// = row i of fgpu_expand over the same arguments is not empty.  The chain up to the last hop runs as in the probe; the last hop
// is never expanded (exists.hip): it settles every row that reaches a destination no tombstone can mask, and the rows that only
// reach columns of the last dm — where the row-level mask of Matrix::delta_lmxm decides — go through the whole chain once more,
// those rows alone.
fgpu_info fgpu_expand_exists(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m, const fgpu_mat* const* dp,
                             const fgpu_mat* const* dm, int nhops, const uint64_t* dst_label_bitmap, uint64_t* match_bits, uint64_t* flops,
                             uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && match_bits && (nsrc == 0 || src_ids), FGPU_NULL_POINTER, "fgpu_expand_exists: NULL argument");
    if (flops) *flops = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    const Layers L{m, dp, dm, nhops};
    FGPU_TRY(check_hops(L, nsrc));
    if (nsrc == 0) return FGPU_OK;
    const u32 k = (u32)nsrc, kw = (k + 63) / 64;
    memset(match_bits, 0, (size_t)kw * sizeof(uint64_t));
    const fgpu_mat *ml = m[nhops - 1], *dpl = L.dp_at(nhops - 1), *dml = L.dm_at(nhops - 1);
    // the chain up to the last hop: a sorted-CSR frontier (f), or the bit state it ended in (bs)
    ChainResult res;
    if (nhops == 1) FGPU_TRY(upload_sources(ctx, &res.mat.m, src_ids, nsrc, m[0]->nrows));
    else FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops - 1}, nullptr, flops, ChainEnd::Bits}, res));
    const fgpu_mat* f = res.kind == ChainResult::Bits ? nullptr : res.mat.get();
    BitState& bs = res.bits;
    DevBuf<u64> bm, out;
    FGPU_TRY(label_to_device(ctx, dst_label_bitmap, ml->ncols, bm));
    const u32 words = f ? kw : (bs.w > kw ? bs.w : kw);          // sure, then maybe
    FGPU_TRY(out.alloc(ctx, (size_t)2 * words));
    FGPU_HIP(hipMemsetAsync(out.p, 0, (size_t)2 * words * sizeof(u64), ctx->stream()));
    u64 entries = 0;
    const fgpu_info ei = exists_rows(ctx, f, f ? nullptr : &bs, ml, dpl, dml, bm.p, k, out.p, out.p + words, words, &entries);
    std::vector<u64> h((size_t)2 * words);
    std::vector<u32> rank;
    fgpu_info di = ei;
    if (di == FGPU_OK) di = ctx->d2h(h.data(), out.p, h.size() * sizeof(u64));
    if (di == FGPU_OK && !f && bs.nsrc_full) {
        rank.resize((size_t)bs.nsrc_full + 1);
        di = ctx->d2h(rank.data(), bs.rowrank.p, rank.size() * sizeof(u32));
    }
    if (!f) bp_finish(ctx, bs);
    FGPU_TRY(di);
    // bit j of a compacted state is live row j: source row i is live (rank[i + 1] > rank[i]) or was dropped as empty
    std::vector<u64> src_left;
    std::vector<u32> row_left;
    u64 matched = 0;
    for (u32 i = 0; i < k; ++i) {
        u32 j = i;
        if (!rank.empty()) {
            if (rank[i + 1] == rank[i]) continue;
            j = rank[i];
        }
        if (src_ids[i] == UINT64_MAX) continue;
        const u64 bit = 1ull << (j & 63);
        if (h[j >> 6] & bit) { match_bits[i >> 6] |= 1ull << (i & 63); ++matched; }
        else if (h[words + (j >> 6)] & bit) { src_left.push_back(src_ids[i]); row_left.push_back(i); }
    }
    if (!src_left.empty()) {
        // the undecided rows: every destination they reach is a column of dm, so only the row-level mask tells — the chain
        // itself, over these rows alone, and its row pointers
        ChainResult ex;
        FGPU_TRY(expand_device(ctx, {src_left.data(), src_left.size(), {m, dp, dm, nhops}, dst_label_bitmap, nullptr, ChainEnd::Csr}, ex));
        const fgpu_mat* r = ex.mat.get();
        const u32 nl = (u32)src_left.size();
        if (r->nnz) {
            if (r->is_hyper()) {
                std::vector<u32> hr(r->nvec), srp((size_t)r->nvec + 1);
                FGPU_TRY(ctx->d2h(srp.data(), r->rowptr, srp.size() * sizeof(u32)));
                if (r->nvec) FGPU_TRY(ctx->d2h(hr.data(), r->hrows, (size_t)r->nvec * sizeof(u32)));
                for (u32 q = 0; q < r->nvec; ++q)
                    if (srp[q + 1] > srp[q] && hr[q] < nl) { match_bits[row_left[hr[q]] >> 6] |= 1ull << (row_left[hr[q]] & 63); ++matched; }
            } else {
                std::vector<u32> rp((size_t)nl + 1);
                FGPU_TRY(ctx->d2h(rp.data(), r->rowptr, rp.size() * sizeof(u32)));
                for (u32 q = 0; q < nl; ++q)
                    if (rp[q + 1] > rp[q]) { match_bits[row_left[q] >> 6] |= 1ull << (row_left[q] & 63); ++matched; }
            }
        }
    }
    if (stats) { stats[0] = matched; stats[1] = src_left.size(); stats[2] = entries; stats[3] = f ? 0 : 1; }
    return FGPU_OK;
}

// ---- streamed result (include/fgpu.h fgpu_expand_stream_*) ----------------------------------------------------------
struct fgpu_expand_stream {
    static constexpr int NS = 4;
    fgpu_ctx* ctx = nullptr;
    hipStream_t st = nullptr;        // the opening thread's lane
    MatRef r;                        // F on the device
    std::vector<u32> rp;             // its row pointers (nsrc + 1)
    u64 nsrc = 0, chunk_rows = 0;
    int width = 8;                   // bytes per destination id handed out
    size_t cap = 0;                  // entries per slot
    struct Slot {
        void* host = nullptr;        // pinned, cap * width bytes
        DevBuf<u64> wide;            // device staging of the widened ids (width 8)
        std::vector<u64> rowptr;     // relative offsets of the chunk's rows
        hipEvent_t ev = nullptr;
        u64 first = 0, nrows = 0;
    } slot[NS];
    u64 enq_row = 0;                 // first row not yet enqueued
    int head = 0, inflight = 0;      // slot of the oldest enqueued chunk; chunks enqueued and not yet handed out
    bool held = false;               // the caller is reading slot (head - 1)
};

static fgpu_info stream_enqueue(fgpu_expand_stream* s, int k) {
    auto& sl = s->slot[k];
    const u64 first = s->enq_row;
    const u64 nr = s->nsrc - first < s->chunk_rows ? s->nsrc - first : s->chunk_rows;
    const u64 b = s->rp[first], e = s->rp[first + nr], n = e - b;
    sl.first = first; sl.nrows = nr;
    sl.rowptr.resize(nr + 1);
    for (u64 i = 0; i <= nr; ++i) sl.rowptr[i] = (u64)s->rp[first + i] - b;
    if (n) {
        if (s->width == 8) {
            FGPU_TRY(fgpu::widen_on_device(s->ctx, sl.wide.p, s->r->colidx + b, n));
            FGPU_HIP(hipMemcpyAsync(sl.host, sl.wide.p, n * 8, hipMemcpyDeviceToHost, s->st));
        } else {
            FGPU_HIP(hipMemcpyAsync(sl.host, s->r->colidx + b, n * 4, hipMemcpyDeviceToHost, s->st));
        }
    }
    FGPU_HIP(hipEventRecord(sl.ev, s->st));
    s->enq_row = first + nr;
    ++s->inflight;
    return FGPU_OK;
}

fgpu_info fgpu_expand_stream_close(fgpu_expand_stream* s) {
    if (!s) return FGPU_OK;
    fgpu_ctx* ctx = s->ctx;
    if (s->st) (void)hipStreamSynchronize(s->st);
    for (auto& sl : s->slot) {
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        if (sl.host) ctx->host_free(sl.host);
    }
    delete s;   // (and with it the slots' device staging, then the result on the device)
    return FGPU_OK;
}

fgpu_info fgpu_expand_stream_open(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                                  const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                                  const uint64_t* dst_label_bitmap, uint64_t chunk_rows, int dest_bits,
                                  fgpu_expand_stream** out, uint64_t* nnz, uint64_t* flops) {
    FGPU_REQUIRE(ctx && out, FGPU_NULL_POINTER, "fgpu_expand_stream_open: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_stream_open: NULL src_ids");
    FGPU_REQUIRE(dest_bits == 32 || dest_bits == 64, FGPU_INVALID, "fgpu_expand_stream_open: dest_bits must be 32 or 64");
    FGPU_REQUIRE(chunk_rows >= 1, FGPU_INVALID, "fgpu_expand_stream_open: chunk_rows must be >= 1");
    *out = nullptr;
    if (flops) *flops = 0;
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, ChainEnd::Csr}, res));
    fgpu_expand_stream* s = new (std::nothrow) fgpu_expand_stream();
    FGPU_REQUIRE(s != nullptr, FGPU_OOM, "fgpu_expand_stream_open: out of host memory");
    const fgpu_mat* r = res.mat.get();
    s->ctx = ctx; s->st = ctx->stream(); s->r = std::move(res.mat); s->nsrc = nsrc; s->chunk_rows = chunk_rows; s->width = dest_bits / 8;
    fgpu_info i = FGPU_OK;
    s->rp.assign(nsrc + 1, 0);
    if (r->nnz) {
        if (r->is_hyper()) {          // (expand_device returns one stored row per source row; guard the other form)
            std::vector<u32> hr(r->nvec), srp((size_t)r->nvec + 1);
            i = ctx->d2h(srp.data(), r->rowptr, srp.size() * sizeof(u32));
            if (i == FGPU_OK && r->nvec) i = ctx->d2h(hr.data(), r->hrows, (size_t)r->nvec * sizeof(u32));
            if (i == FGPU_OK) {
                for (u32 k = 0; k < r->nvec; ++k) s->rp[hr[k] + 1] = srp[k + 1] - srp[k];
                for (u64 q = 0; q < nsrc; ++q) s->rp[q + 1] += s->rp[q];
            }
        } else {
            i = ctx->d2h(s->rp.data(), r->rowptr, (nsrc + 1) * sizeof(u32));
        }
    }
    if (i == FGPU_OK) {
        for (u64 f = 0; f < nsrc; f += chunk_rows) {
            const u64 l = f + chunk_rows < nsrc ? f + chunk_rows : nsrc;
            const size_t n = (size_t)s->rp[l] - s->rp[f];
            if (n > s->cap) s->cap = n;
        }
        const u64 nchunks = nsrc ? (nsrc + chunk_rows - 1) / chunk_rows : 0;
        const int use = nchunks < (u64)fgpu_expand_stream::NS ? (int)nchunks : fgpu_expand_stream::NS;
        for (int k = 0; k < use && i == FGPU_OK; ++k) {
            auto& sl = s->slot[k];
            sl.host = ctx->pinned_alloc((s->cap ? s->cap : 1) * s->width);
            if (!sl.host) { set_error("fgpu_expand_stream_open: pinned host memory exhausted"); i = FGPU_OOM; break; }
            if (s->width == 8) i = sl.wide.alloc(ctx, s->cap);
            if (i == FGPU_OK && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) {
                set_error("fgpu_expand_stream_open: hipEventCreate failed");
                i = FGPU_DEVICE;
            }
        }
        for (int k = 0; k < use && i == FGPU_OK && s->enq_row < nsrc; ++k) i = stream_enqueue(s, k);
    }
    if (i != FGPU_OK) { fgpu_expand_stream_close(s); return i; }
    if (nnz) *nnz = r->nnz;
    *out = s;
    return FGPU_OK;
}

fgpu_info fgpu_expand_stream_next(fgpu_expand_stream* s, uint64_t* first_row, uint64_t* nrows, const uint64_t** rowptr,
                                  const void** dest) {
    FGPU_REQUIRE(s && first_row && nrows && rowptr && dest, FGPU_NULL_POINTER, "fgpu_expand_stream_next: NULL argument");
    FGPU_REQUIRE(s->ctx->stream() == s->st, FGPU_INVALID, "fgpu_expand_stream_next: a stream belongs to the thread that opened it");
    constexpr int NS = fgpu_expand_stream::NS;
    if (s->held) {                         // the chunk handed out last is done with: its slot takes the next one
        s->held = false;
        const int freed = (s->head + NS - 1) % NS;
        if (s->enq_row < s->nsrc) FGPU_TRY(stream_enqueue(s, freed));
    }
    *nrows = 0; *first_row = s->nsrc; *rowptr = nullptr; *dest = nullptr;
    if (s->inflight == 0) return FGPU_NO_VALUE;
    auto& sl = s->slot[s->head];
    FGPU_HIP(hipEventSynchronize(sl.ev));
    *first_row = sl.first; *nrows = sl.nrows; *rowptr = sl.rowptr.data(); *dest = sl.host;
    s->head = (s->head + 1) % NS;
    --s->inflight;
    s->held = true;
    return FGPU_OK;
}

fgpu_info fgpu_expand32(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                        const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                        const uint64_t* dst_label_bitmap, uint32_t** out_rowptr, uint32_t** out_dest,
                        uint64_t* out_nnz, uint64_t* flops) {
    FGPU_REQUIRE(ctx && out_rowptr && out_dest && out_nnz, FGPU_NULL_POINTER, "fgpu_expand32: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand32: NULL src_ids");
    *out_rowptr = nullptr; *out_dest = nullptr; *out_nnz = 0;
    if (flops) *flops = 0;
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, ChainEnd::Csr}, res));
    const fgpu_mat* r = res.mat.get();
    FGPU_REQUIRE(!r->is_hyper() && r->nrows == nsrc, FGPU_INVALID, "fgpu_expand32: the chain's result is not a dense-row CSR");
    // the device arrays as they are: two DMAs into pinned result blocks, nothing widened anywhere
    ResultBuf hrp, hci;
    FGPU_REQUIRE(hrp.alloc(ctx, (nsrc + 1) * sizeof(u32)) && hci.alloc(ctx, (r->nnz ? r->nnz : 1) * sizeof(u32)), FGPU_OOM,
                 "fgpu_expand32: host allocation failed");
    FGPU_TRY(ctx->d2h(hrp.p, r->rowptr, (nsrc + 1) * sizeof(u32)));
    if (r->nnz) FGPU_TRY(ctx->d2h(hci.p, r->colidx, r->nnz * sizeof(u32)));
    *out_rowptr = (u32*)hrp.release(); *out_dest = (u32*)hci.release(); *out_nnz = r->nnz;
    return FGPU_OK;
}

fgpu_info fgpu_expand_mat(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                          const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                          const uint64_t* dst_label_bitmap, fgpu_mat** out, uint64_t* flops) {
    FGPU_REQUIRE(ctx && out, FGPU_NULL_POINTER, "fgpu_expand_mat: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_mat: NULL src_ids");
    if (flops) *flops = 0;
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, ChainEnd::Csr}, res));
    FGPU_TRY(ctx->publish());   // the new handle may go to another thread
    *out = res.mat.release();
    return FGPU_OK;
}

fgpu_info fgpu_expand_count(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                            const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                            const uint64_t* dst_label_bitmap, uint64_t* out_nnz, uint64_t* checksum,
                            uint64_t* flops) {
    FGPU_REQUIRE(ctx && out_nnz, FGPU_NULL_POINTER, "fgpu_expand_count: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_count: NULL src_ids");
    if (flops) *flops = 0;
    if (ctx->opt.expand_scan_min > 0 && nsrc > (u64)ctx->opt.expand_scan_min && ctx->opt.expand_mode != 1)
        return expand_count_scan(ctx, src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, out_nnz, checksum, flops);
    ChainResult res;
    FGPU_TRY(expand_device(ctx, {src_ids, nsrc, {m, dp, dm, nhops}, dst_label_bitmap, flops, checksum ? ChainEnd::CountSum : ChainEnd::Count},
                           res));
    if (res.kind == ChainResult::Counts) {   // the chain ended in bit form: counted there, no CSR was materialized
        *out_nnz = res.nnz;
        if (checksum) *checksum = res.checksum;
        return FGPU_OK;
    }
    return count_csr_result(ctx, res.mat.get(), nullptr, nullptr, out_nnz, checksum);
}

fgpu_info fgpu_expand_levels(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc, const fgpu_mat* const* m,
                             const fgpu_mat* const* dp, const fgpu_mat* const* dm, int nhops,
                             const uint64_t* dst_label_bitmap, uint64_t* hop_nnz, uint64_t* hop_checksum,
                             uint64_t* union_nnz, uint64_t* union_checksum, uint64_t* flops) {
    FGPU_REQUIRE(ctx && hop_nnz, FGPU_NULL_POINTER, "fgpu_expand_levels: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_levels: NULL src_ids");
    const Layers L{m, dp, dm, nhops};
    FGPU_TRY(check_hops(L, nsrc));
    for (int h = 0; h < nhops; ++h)
        FGPU_REQUIRE(!m[h]->is_hyper() && m[h]->nnz < 0x7FFFFFFFull, FGPU_INVALID,
                     "fgpu_expand_levels: hop %d needs a non-hypersparse base matrix with nnz < 2^31", h);
    if (flops) *flops = 0;
    if (union_nnz) *union_nnz = 0;
    if (union_checksum) *union_checksum = 0;
    MatRef f;
    FGPU_TRY(upload_sources(ctx, &f.m, src_ids, nsrc, m[0]->nrows));
    // the whole chain runs in bit form (one bit per source row): every hop is one pass over the cached
    // transpose whatever the frontier size, and the union over the hops is a word-wise OR
    BitState bs, un;
    FGPU_TRY(bp_from_csr(ctx, bs, f.get()));
    f.reset();
    DevBuf<u64> bm;
    for (int h = 0; h < nhops; ++h) {
        FGPU_TRY(bp_hop(ctx, bs, m[h], L.dp_at(h), L.dm_at(h), flops));
        if (h == 0) FGPU_TRY(label_to_device(ctx, dst_label_bitmap, bs.n, bm));   // the destination label applies to every reported set
        const u64* label_dev = bm.p;
        u64 n = 0, cs = 0;
        FGPU_TRY(bp_count(ctx, bs, label_dev, &n, hop_checksum ? &cs : nullptr));
        hop_nnz[h] = n;
        if (hop_checksum) hop_checksum[h] = cs;
        if (union_nnz || union_checksum) FGPU_TRY(bp_accumulate(ctx, un, bs));
    }
    if (union_nnz || union_checksum) {
        u64 n = 0, cs = 0;
        FGPU_TRY(bp_count(ctx, un, bm.p, &n, union_checksum ? &cs : nullptr));
        if (union_nnz) *union_nnz = n;
        if (union_checksum) *union_checksum = cs;
    }
    bp_finish(ctx, bs);
    return FGPU_OK;
}

}  // extern "C"

extern "C" fgpu_info fgpu_expand_trail_counts(fgpu_ctx* ctx, const uint64_t* src_ids, uint64_t nsrc,
                                              const fgpu_mat* const* m, const fgpu_mat* const* dp,
                                              const fgpu_mat* const* dm, int nhops, int weighted,
                                              uint64_t** out_rowptr, uint64_t** out_dest, uint64_t** out_count,
                                              uint64_t* out_nnz) {
    FGPU_REQUIRE(ctx && out_rowptr && out_dest && out_count && out_nnz, FGPU_NULL_POINTER, "fgpu_expand_trail_counts: NULL argument");
    FGPU_REQUIRE(nsrc == 0 || src_ids, FGPU_NULL_POINTER, "fgpu_expand_trail_counts: NULL src_ids");
    FGPU_REQUIRE(nhops == 1 || nhops == 2, FGPU_INVALID,
                 "fgpu_expand_trail_counts: trail counts have a product form for 1 or 2 hops only (cond_var_len_traverse.rs keeps the DFS beyond)");
    const Layers L{m, dp, dm, nhops};
    FGPU_TRY(check_hops(L, nsrc));
    for (u64 i = 0; i < nsrc; ++i)
        FGPU_REQUIRE(src_ids[i] != UINT64_MAX, FGPU_INVALID, "fgpu_expand_trail_counts: every row needs a source");
    // `-[:T*1..2]->` walks ONE relationship: the "same edge twice" correction of the two-hop count (the a -> a -> a walk
    // over one self-loop) is only meaningful when both hops read the same layers.  With different layers per hop no
    // edge can repeat and the subtraction would undercount, so that form is refused rather than answered wrongly.
    FGPU_REQUIRE(nhops == 1 || (m[0] == m[1] && L.dp_at(0) == L.dp_at(1) && L.dm_at(0) == L.dm_at(1)),
                 FGPU_INVALID, "fgpu_expand_trail_counts: both hops must read the same relationship layers (one var-length relationship)");
    // effective layers (m \ dm) U dp — real edges, no row-level mask quirk: these are counts of paths, not a delta_lmxm
    std::vector<const fgpu_mat*> eff(nhops, nullptr);
    std::vector<MatRef> owned;
    for (int h = 0; h < nhops; ++h) {
        const fgpu_mat *dph = L.dp_at(h), *dmh = L.dm_at(h);
        const bool dirty = (dph && dph->nnz) || (dmh && dmh->nnz);
        if (!dirty && !m[h]->is_hyper()) { eff[h] = m[h]; continue; }
        MatRef e;
        FGPU_TRY(mat_merge_entries(ctx, &e.m, m[h], dph, dmh, false, m[h]->nrows, m[h]->ncols, !weighted));
        eff[h] = e.get();
        owned.push_back(std::move(e));
    }
    if (weighted)
        for (int h = 0; h < nhops; ++h)
            FGPU_REQUIRE(eff[h]->vals, FGPU_INVALID, "fgpu_expand_trail_counts: weighted counts need UINT64 multiplicity layers");
    MatRef f0, c1, c2;
    DevBuf<u32> dsrc;
    DevBuf<u64> w1, cnt;
    std::vector<u32> s32(nsrc);
    for (u64 k = 0; k < nsrc; ++k) s32[k] = (u32)src_ids[k];
    FGPU_TRY(upload_sources(ctx, &f0.m, src_ids, nsrc, eff[0]->nrows));
    FGPU_TRY(dsrc.alloc(ctx, nsrc));
    FGPU_TRY(ctx->h2d(dsrc.p, s32.data(), nsrc * sizeof(u32)));
    FGPU_TRY(mxm_device(ctx, &c1.m, f0.get(), eff[0], nullptr));
    FGPU_TRY(w1.alloc(ctx, c1->nnz));
    if (c1->nnz) {
        u32 grid = cdiv(nsrc, 4);
        if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
        FGPU_TRY(launch(row_weight_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(c1.get()), view_of(eff[0]),
                        weighted ? (const u64*)eff[0]->vals : (const u64*)nullptr, (const u32*)dsrc.p, (u32)nsrc, w1.p));
    }
    const fgpu_mat* res = c1.get();
    const u64* res_cnt = w1.p;
    if (nhops == 2) {
        FGPU_TRY(mxm_device(ctx, &c2.m, c1.get(), eff[1], nullptr));
        FGPU_TRY(cnt.alloc(ctx, c2->nnz));
        FGPU_HIP(hipMemsetAsync(cnt.p, 0, (size_t)(c2->nnz ? c2->nnz : 1) * sizeof(u64), ctx->stream()));
        if (c1->nnz && c2->nnz) {
            u32 grid = cdiv(c1->nnz, 4);
            if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
            FGPU_TRY(launch(trail2_count_kernel, dim3(grid), dim3(256), 0, ctx->stream(), view_of(c1.get()), (const u64*)w1.p,
                            view_of(eff[1]), weighted ? (const u64*)eff[1]->vals : (const u64*)nullptr, view_of(c2.get()),
                            (const u32*)dsrc.p, (u32)c1->nnz, (unsigned long long*)cnt.p));
        }
        res = c2.get();
        res_cnt = cnt.p;
    }
    // host hand-over: rowptr / dest as fgpu_expand does, counts beside them.  Pairs reached only through the
    // self-loop walk keep a zero count: they are walks, not trails, and are dropped here.
    std::vector<u32> rp((size_t)nsrc + 1), ci(res->nnz);
    std::vector<u64> cv(res->nnz);
    FGPU_TRY(ctx->d2h(rp.data(), res->rowptr, rp.size() * sizeof(u32)));
    if (res->nnz) {
        FGPU_TRY(ctx->d2h(ci.data(), res->colidx, res->nnz * sizeof(u32)));
        FGPU_TRY(ctx->d2h(cv.data(), res_cnt, res->nnz * sizeof(u64)));
    }
    FGPU_HIP(hipStreamSynchronize(ctx->stream()));
    u64 keep = 0;
    for (u64 k = 0; k < res->nnz; ++k) keep += cv[k] != 0;
    ResultBuf brp, bd, bc;   // (the caller's allocator, not pinned result blocks)
    FGPU_REQUIRE(brp.alloc_host(ctx, (nsrc + 1) * sizeof(u64)) && bd.alloc_host(ctx, (keep ? keep : 1) * sizeof(u64)) &&
                     bc.alloc_host(ctx, (keep ? keep : 1) * sizeof(u64)),
                 FGPU_OOM, "fgpu_expand_trail_counts: host allocation failed");
    u64 *orp = (u64*)brp.release(), *od = (u64*)bd.release(), *oc = (u64*)bc.release();   // nothing below can fail
    u64 o = 0;
    for (u64 r = 0; r < nsrc; ++r) {
        orp[r] = o;
        for (u32 k = rp[r]; k < rp[r + 1]; ++k)
            if (cv[k]) { od[o] = ci[k]; oc[o] = cv[k]; ++o; }
    }
    orp[nsrc] = o;
    *out_rowptr = orp; *out_dest = od; *out_count = oc; *out_nnz = o;
    return FGPU_OK;
}

// Public producers of snapshots: the implementation above, then fgpu_ctx::publish().
extern "C" {

fgpu_info fgpu_mxm(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* b) {
    fgpu_info i_ = mxm_impl(ctx, c, f, b);
    if (i_ == FGPU_OK && ctx) i_ = ctx->publish();   // the new handle may go to another thread
    return i_;
}

fgpu_info fgpu_delta_lmxm(fgpu_ctx* ctx, fgpu_mat** c, const fgpu_mat* f, const fgpu_mat* m, const fgpu_mat* dp,
                          const fgpu_mat* dm) {
    fgpu_info i_ = delta_lmxm_impl(ctx, c, f, m, dp, dm);
    if (i_ == FGPU_OK && ctx) i_ = ctx->publish();   // the new handle may go to another thread
    return i_;
}

}  // extern "C"
