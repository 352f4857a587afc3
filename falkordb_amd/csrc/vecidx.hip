// vecidx.hip — exhaustive vector similarity search (fgpu_vecidx_*): the device core of db.idx.vector.queryNodes /
// queryRelationships.  The rules are in include/fgpu.h; this file is the store, the scoring GEMM and the selection.
//
// Layout.  A vector lives in a SLOT; 16 consecutive slots are a row tile and 16 consecutive components a k-chunk.  One
// (tile, chunk) block is 256 floats in exactly the order a wavefront feeds v_mfma_f32_16x16x4_f32 with: lane l = 16 h + r
// owns the float4 { x[r][16 c + 4 s + h] : s = 0 .. 3 }, so one coalesced 16-byte load per lane is the A (or B) operand of
// the chunk's four MFMAs, step s summing k = 16 c + 4 s + 0 .. 3.  Queries are packed the same way.  dim is padded to whole
// chunks and the last tile to 16 rows with zeros: a zero product leaves an fmaf chain as it was, so S(q, x) is the chain
// over the real components, and no load leaves the allocation.
//
// Scoring.  A wavefront owns one row tile and NQT (1, 2 or 4) query tiles: per chunk one load of the store feeds 4 NQT
// MFMAs.  K is never split: every accumulator element is one k-ordered chain from 0, whatever nq is.  The epilogue turns S
// into the metric's f32 key and stores its order-preserving u32 image.
//
// Selection.  Per query an 8-pass, 8-bit radix select over the 64-bit value (key image << 32 | id) finds the kk-th smallest
// (key, id); the last four passes, the ones over the id, are skipped when the ties at the kk-th key all fit.  One more pass
// compacts the entries at or below it, and a last kernel computes their FP64 distances.
#include <math.h>

#include <algorithm>
#include <unordered_map>
#include <unordered_set>

#include "common.hpp"

namespace fgpu {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr u32 VT = 16;                          // rows per tile, components per chunk
constexpr size_t SCORE_BUDGET = 256ull << 20;   // bytes of key images per chunk of queries
constexpr u32 SEL_PER_WG = 8192;                // entries a workgroup of the selection passes reads
constexpr u64 SEL_QUERIES_MAX = 4096;           // queries per chunk at most (they are the y dimension of the selection grids)

// the float of component k of slot s inside a blocked array of `nch` chunks per tile
__host__ __device__ __forceinline__ size_t blk_off(u32 s, u32 k, u32 nch) {
    return ((size_t)(s >> 4) * nch + (k >> 4)) * 256 + (((k & 3) * 16 + (s & 15)) * 4 + ((k >> 2) & 3));
}

// rows of `src` (row-major, `dim` floats each) into their slots of the blocked array; a thread per (row, chunk, h) float4
__global__ __launch_bounds__(256) void vec_pack_kernel(const float* __restrict__ src, const u32* __restrict__ src_row,
                                                      const u32* __restrict__ slot, u64 nwin, u32 dim, u32 nch,
                                                      float* __restrict__ blk) {
    const u64 total = nwin * nch * 4;
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < total; t += (u64)gridDim.x * 256) {
        const u32 h = (u32)(t & 3);
        const u32 c = (u32)((t >> 2) % nch);
        const u64 w = (t >> 2) / nch;
        const u32 s = slot ? slot[w] : (u32)w;
        const float* row = src + (size_t)(src_row ? src_row[w] : (u32)w) * dim;
        float4 v;
        const u32 k0 = 16 * c + h;
        v.x = k0 < dim ? row[k0] : 0.0f;
        v.y = k0 + 4 < dim ? row[k0 + 4] : 0.0f;
        v.z = k0 + 8 < dim ? row[k0 + 8] : 0.0f;
        v.w = k0 + 12 < dim ? row[k0 + 12] : 0.0f;
        *(float4*)(blk + blk_off(s, k0, nch)) = v;
    }
}

// norm[slot] = the fmaf chain of x . x from 0 over the components in index order
__global__ __launch_bounds__(256) void vec_norm_kernel(const float* __restrict__ src, const u32* __restrict__ src_row,
                                                      const u32* __restrict__ slot, u64 nwin, u32 dim,
                                                      float* __restrict__ norm) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (u64)gridDim.x * 256) {
        const float* row = src + (size_t)(src_row ? src_row[w] : (u32)w) * dim;
        float a = 0.0f;
        for (u32 k = 0; k < dim; ++k) a = fmaf(row[k], row[k], a);
        norm[slot ? slot[w] : (u32)w] = a;
    }
}

__global__ __launch_bounds__(256) void vec_ids_kernel(const u32* __restrict__ id, const u32* __restrict__ slot, u64 nwin,
                                                     u32* __restrict__ ids) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (u64)gridDim.x * 256) ids[slot[w]] = id[w];
}

// remove: slot from[m] moves to slot to[m]; every from is at or past the new count and every to below it
__global__ __launch_bounds__(256) void vec_move_kernel(const u32* __restrict__ from, const u32* __restrict__ to, u32 nmoves,
                                                      u32 nch, float* __restrict__ blk, float* __restrict__ norm,
                                                      u32* __restrict__ ids) {
    const u32 dimp = nch * 16;
    const u64 total = (u64)nmoves * dimp;
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < total; t += (u64)gridDim.x * 256) {
        const u32 m = (u32)(t / dimp), k = (u32)(t % dimp);
        blk[blk_off(to[m], k, nch)] = blk[blk_off(from[m], k, nch)];
        if (k == 0) { norm[to[m]] = norm[from[m]]; ids[to[m]] = ids[from[m]]; }
    }
}

__global__ __launch_bounds__(256) void vec_get_kernel(const float* __restrict__ blk, u32 slot, u32 dim, u32 nch,
                                                     float* __restrict__ out) {
    for (u32 k = blockIdx.x * 256 + threadIdx.x; k < dim; k += gridDim.x * 256) out[k] = blk[blk_off(slot, k, nch)];
}

// the order-preserving u32 image of an f32 key; -0.0 and +0.0 share one, and a NaN (finite components whose sums overflowed:
// inf - inf, 0 / 0) gets the largest, after +inf
__device__ __forceinline__ u32 key_image(float key) {
    if (key != key) return 0xFFFFFFFFu;
    if (key == 0.0f) key = 0.0f;
    const u32 b = __float_as_uint(key);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float vec_key(int metric, float s, float nq, float nx) {
    if (metric == FGPU_VEC_EUCLIDEAN) {
        const float t = nq + nx;
        return t - 2.0f * s;
    }
    if (metric == FGPU_VEC_IP) return -s;
    if (nq == 0.0f || nx == 0.0f) return 1.0f;
    return 1.0f - s / (__fsqrt_rn(nq) * __fsqrt_rn(nx));
}

// one k-chunk: step s of the four sums k = 16 c + 4 s + 0 .. 3 on top of acc
__device__ __forceinline__ f32x4 chunk_mfma(float4 a, float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// scores[q][row] for one row tile and NQT query tiles per wavefront; grid.y = groups of NQT query tiles
template <int NQT>
__global__ __launch_bounds__(256) void vec_score_kernel(const float4* __restrict__ store, const float4* __restrict__ qblk,
                                                       const float* __restrict__ nx, const float* __restrict__ nq,
                                                       u32* __restrict__ scores, u32 ntiles, u32 nch, u32 stride, int metric) {
    const u32 lane = threadIdx.x & 63;
    const u32 qt0 = blockIdx.y * NQT;
    const float4* b[NQT];
#pragma unroll
    for (int j = 0; j < NQT; ++j) b[j] = qblk + (size_t)(qt0 + j) * nch * 64 + lane;
    for (u32 t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * 4) {
        const float4* a = store + (size_t)t * nch * 64 + lane;
        f32x4 acc[NQT];
#pragma unroll
        for (int j = 0; j < NQT; ++j) acc[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        u32 c = 0;
        for (; c + 2 <= nch; c += 2) {   // two chunks of the store in flight per wavefront; the chain stays in k order
            const float4 av0 = a[(size_t)c * 64], av1 = a[(size_t)(c + 1) * 64];
#pragma unroll
            for (int j = 0; j < NQT; ++j) {
                const float4 bv0 = b[j][(size_t)c * 64], bv1 = b[j][(size_t)(c + 1) * 64];
                acc[j] = chunk_mfma(av0, bv0, acc[j]);
                acc[j] = chunk_mfma(av1, bv1, acc[j]);
            }
        }
        if (c < nch) {
            const float4 av = a[(size_t)c * 64];
#pragma unroll
            for (int j = 0; j < NQT; ++j) acc[j] = chunk_mfma(av, b[j][(size_t)c * 64], acc[j]);
        }
        // D: column (query) = lane & 15, rows (slots) = 4 (lane >> 4) + 0 .. 3
        const u32 r0 = t * 16 + (lane >> 4) * 4;
        const float4 xn = *(const float4*)(nx + r0);
#pragma unroll
        for (int j = 0; j < NQT; ++j) {
            const u32 q = (qt0 + j) * 16 + (lane & 15);
            const float qn = nq[q];
            uint4 o;
            o.x = key_image(vec_key(metric, acc[j][0], qn, xn.x));
            o.y = key_image(vec_key(metric, acc[j][1], qn, xn.y));
            o.z = key_image(vec_key(metric, acc[j][2], qn, xn.z));
            o.w = key_image(vec_key(metric, acc[j][3], qn, xn.w));
            *(uint4*)(scores + (size_t)q * stride + r0) = o;
        }
    }
}

struct VecSel {      // per query
    u64 prefix;      // the digits of the kk-th smallest (image << 32 | id) found so far
    u32 kleft;       // its rank among the entries that share them
    u32 done;        // the id passes are not needed: every tie fits
    u32 ties;        // entries whose key is the kk-th key
    u32 out;         // compaction cursor
};

__global__ __launch_bounds__(256) void vec_sel_init_kernel(VecSel* __restrict__ sel, u32* __restrict__ hist, u32 nq, u32 kk) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < nq * 256) hist[i] = 0;
    if (i < nq) { sel[i].prefix = 0; sel[i].kleft = kk; sel[i].done = 0; sel[i].ties = 0; sel[i].out = 0; }
}

__device__ __forceinline__ u64 sel_value(u32 img, u32 want_img, const u32* __restrict__ ids, u32 i) {
    return ((u64)img << 32) | (img == want_img ? ids[i] : 0u);
}

// histogram of the digit at `shift` over the entries that share the digits above it; grid = (parts, queries)
__global__ __launch_bounds__(256) void vec_sel_hist_kernel(const u32* __restrict__ scores, const u32* __restrict__ ids,
                                                          const VecSel* __restrict__ sel, u32* __restrict__ hist, u32 count,
                                                          u32 stride, u32 shift) {
    __shared__ u32 s_h[256];
    const u32 q = blockIdx.y;
    if (sel[q].done) return;
    const u64 prefix = sel[q].prefix;
    const u32 want = shift < 32 ? (u32)(prefix >> 32) : 0xFFFFFFFFu;   // ids are read in the id passes, for the ties only
    const bool with_id = shift < 32;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const u32* row = scores + (size_t)q * stride;
    const u32 base = blockIdx.x * SEL_PER_WG;
    for (u32 i0 = base + threadIdx.x * 4; i0 < base + SEL_PER_WG && i0 < count; i0 += 1024) {
        const uint4 v = *(const uint4*)(row + i0);   // (stride is a multiple of 16: the load stays inside the row)
        const u32 img[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 e = 0; e < 4; ++e) {
            if (i0 + e >= count) break;
            if (with_id && img[e] != want) continue;
            const u64 val = with_id ? sel_value(img[e], want, ids, i0 + e) : (u64)img[e] << 32;
            if ((((val ^ prefix) >> shift) >> 8) == 0) atomicAdd(&s_h[(u32)(val >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&hist[q * 256 + threadIdx.x], s_h[threadIdx.x]);
}

// the digit holding rank kleft; one workgroup per query.  After the last image pass (shift 32) the ties are known.
__global__ __launch_bounds__(256) void vec_sel_pick_kernel(VecSel* __restrict__ sel, u32* __restrict__ hist, u32 shift) {
    __shared__ u32 s_c[256];
    const u32 q = blockIdx.x, d = threadIdx.x;
    if (sel[q].done) return;
    const u32 h = hist[q * 256 + d];
    hist[q * 256 + d] = 0;
    const u32 kleft = sel[q].kleft;
    const u64 prefix = sel[q].prefix;
    s_c[d] = h;
    __syncthreads();
    for (u32 o = 1; o < 256; o <<= 1) {   // inclusive scan
        const u32 add = d >= o ? s_c[d - o] : 0;
        __syncthreads();
        s_c[d] += add;
        __syncthreads();
    }
    const u32 excl = s_c[d] - h;
    if (excl < kleft && kleft <= excl + h) {   // exactly one digit: 1 <= kleft <= the entries counted
        u64 p = prefix | ((u64)d << shift);
        const u32 left = kleft - excl;
        if (shift == 32) {
            sel[q].ties = h;
            if (h == left) { sel[q].done = 1; p |= 0xFFFFFFFFull; }
        }
        sel[q].prefix = p;
        sel[q].kleft = left;
    }
}

// the entries at or below the kk-th (key, id), in any order; tie_total += the ties the id order had to decide
__global__ __launch_bounds__(256) void vec_sel_compact_kernel(const u32* __restrict__ scores, const u32* __restrict__ ids,
                                                             VecSel* __restrict__ sel, u32 count, u32 stride, u32 kk,
                                                             u32* __restrict__ out_slot, unsigned long long* __restrict__ tie_total) {
    const u32 q = blockIdx.y;
    const u64 thr = sel[q].prefix;
    const u32 want = (u32)(thr >> 32);
    const u32* row = scores + (size_t)q * stride;
    const u32 base = blockIdx.x * SEL_PER_WG;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !sel[q].done) atomicAdd(tie_total, (unsigned long long)sel[q].ties);
    for (u32 i0 = base + threadIdx.x * 4; i0 < base + SEL_PER_WG && i0 < count; i0 += 1024) {
        const uint4 v = *(const uint4*)(row + i0);
        const u32 img[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 e = 0; e < 4; ++e) {
            if (i0 + e >= count) break;
            if (img[e] > want) continue;
            if (sel_value(img[e], want, ids, i0 + e) <= thr) {
                const u32 pos = atomicAdd(&sel[q].out, 1u);
                if (pos < kk) out_slot[(size_t)q * kk + pos] = i0 + e;
            }
        }
    }
}

// D(q, x) in FP64 from the stored f32 components, accumulated in index order; a thread per survivor
__global__ __launch_bounds__(256) void vec_dist_kernel(const float* __restrict__ store, const float* __restrict__ qblk,
                                                      const u32* __restrict__ ids, const u32* __restrict__ out_slot, u64 total,
                                                      u32 kk, u32 nch, int metric, double* __restrict__ dist,
                                                      u64* __restrict__ out_id) {
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < total; t += (u64)gridDim.x * 256) {
        const u32 q = (u32)(t / kk), s = out_slot[t];
        double acc = 0.0, qq = 0.0, xx = 0.0;
        for (u32 c = 0; c < nch; ++c) {
            float xv[16], qv[16];
#pragma unroll
            for (u32 h = 0; h < 4; ++h) {   // float4 h of the chunk holds k = 16 c + 4 e + h, e = 0 .. 3
                const float4 x4 = *(const float4*)(store + blk_off(s, 16 * c + h, nch));
                const float4 q4 = *(const float4*)(qblk + blk_off(q, 16 * c + h, nch));
                xv[h] = x4.x; xv[4 + h] = x4.y; xv[8 + h] = x4.z; xv[12 + h] = x4.w;
                qv[h] = q4.x; qv[4 + h] = q4.y; qv[8 + h] = q4.z; qv[12 + h] = q4.w;
            }
#pragma unroll
            for (u32 k = 0; k < 16; ++k) {   // (the zero fill past dim adds +0.0: the sums stay as they are)
                const double x = (double)xv[k], y = (double)qv[k];
                if (metric == FGPU_VEC_EUCLIDEAN) { const double d = y - x; acc += d * d; }
                else {
                    acc += y * x;
                    if (metric == FGPU_VEC_COSINE) { qq += y * y; xx += x * x; }
                }
            }
        }
        double d;
        if (metric == FGPU_VEC_EUCLIDEAN) d = sqrt(acc);
        else if (metric == FGPU_VEC_IP) d = -acc;
        else d = (qq == 0.0 || xx == 0.0) ? 1.0 : 1.0 - acc / (sqrt(qq) * sqrt(xx));
        dist[t] = d;
        out_id[t] = ids[s];
    }
}

inline u32 grid_for(fgpu_ctx* ctx, u64 items, u32 per_wg, u32 per_cu) {
    u64 g = (items + per_wg - 1) / per_wg;
    const u64 cap = (u64)(ctx->cus > 0 ? ctx->cus : 1) * per_cu;
    if (g > cap) g = cap;
    return g ? (u32)g : 1;
}

bool all_finite(const float* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace
}  // namespace fgpu

using namespace fgpu;

struct fgpu_vecidx {
    fgpu_ctx* ctx = nullptr;
    u32 dim = 0, nch = 0;
    int metric = 0;
    u32 count = 0, cap = 0;                  // slots in use, slots allocated (a multiple of 16)
    std::unordered_map<u32, u32> slot_of;    // id -> slot
    std::vector<u32> id_of;                  // slot -> id (host copy of `ids`)
    DevBuf<float> store;                     // cap / 16 tiles of nch blocks of 256 floats
    DevBuf<float> norm;                      // cap: the f32 chain of x . x
    DevBuf<u32> ids;                         // cap
};

namespace {

// capacity for at least `need` slots: doubled, the old content copied, the rest zero
fgpu_info vec_reserve(fgpu_ctx* ctx, fgpu_vecidx* x, u64 need) {
    if (need <= x->cap) return FGPU_OK;
    u64 cap = x->cap ? x->cap : 256;
    while (cap < need) cap *= 2;
    FGPU_REQUIRE(cap < (1ull << 32), FGPU_INVALID, "fgpu_vecidx_set: the store is full");
    hipStream_t st = ctx->stream();
    DevBuf<float> store, norm;
    DevBuf<u32> ids;
    const size_t tile_floats = (size_t)x->nch * 256;
    FGPU_TRY(store.alloc(ctx, cap / VT * tile_floats));
    FGPU_TRY(norm.alloc(ctx, cap));
    FGPU_TRY(ids.alloc(ctx, cap));
    FGPU_HIP(hipMemsetAsync(store.p, 0, cap / VT * tile_floats * sizeof(float), st));
    FGPU_HIP(hipMemsetAsync(norm.p, 0, cap * sizeof(float), st));
    FGPU_HIP(hipMemsetAsync(ids.p, 0, cap * sizeof(u32), st));
    if (x->cap) {
        FGPU_HIP(hipMemcpyAsync(store.p, x->store.p, x->cap / VT * tile_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
        FGPU_HIP(hipMemcpyAsync(norm.p, x->norm.p, x->cap * sizeof(float), hipMemcpyDeviceToDevice, st));
        FGPU_HIP(hipMemcpyAsync(ids.p, x->ids.p, x->cap * sizeof(u32), hipMemcpyDeviceToDevice, st));
    }
    ctx->fence_lanes();   // searches other lanes queued on the old blocks finish before these return to the pool
    x->store = std::move(store);
    x->norm = std::move(norm);
    x->ids = std::move(ids);
    x->cap = (u32)cap;
    return FGPU_OK;
}

}  // namespace

extern "C" {

fgpu_info fgpu_vecidx_new(fgpu_ctx* ctx, fgpu_vecidx** out, uint32_t dim, int metric) {
    FGPU_REQUIRE(ctx && out, FGPU_NULL_POINTER, "fgpu_vecidx_new: NULL argument");
    FGPU_REQUIRE(dim >= 1 && dim <= FGPU_VECIDX_DIM_MAX, FGPU_INVALID, "fgpu_vecidx_new: dim must be 1 .. %d, not %u",
                 FGPU_VECIDX_DIM_MAX, dim);
    FGPU_REQUIRE(metric == FGPU_VEC_EUCLIDEAN || metric == FGPU_VEC_COSINE || metric == FGPU_VEC_IP, FGPU_INVALID,
                 "fgpu_vecidx_new: unknown metric %d", metric);
    fgpu_vecidx* x = new fgpu_vecidx();
    x->ctx = ctx;
    x->dim = dim;
    x->nch = (dim + VT - 1) / VT;
    x->metric = metric;
    *out = x;
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_free(fgpu_vecidx* x) {
    if (!x) return FGPU_OK;
    x->ctx->fence_lanes();   // as fgpu_mat_free: searches other lanes queued finish before the blocks are reused
    delete x;
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_info(const fgpu_vecidx* x, uint32_t* dim, int* metric, uint64_t* count) {
    FGPU_REQUIRE(x, FGPU_NULL_POINTER, "fgpu_vecidx_info: NULL index");
    if (dim) *dim = x->dim;
    if (metric) *metric = x->metric;
    if (count) *count = x->count;
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_set(fgpu_ctx* ctx, fgpu_vecidx* x, const uint64_t* ids, const float* vecs, uint64_t n) {
    FGPU_REQUIRE(ctx && x && (n == 0 || (ids && vecs)), FGPU_NULL_POINTER, "fgpu_vecidx_set: NULL argument");
    if (n == 0) return FGPU_OK;
    FGPU_REQUIRE(n < (1ull << 32), FGPU_INVALID, "fgpu_vecidx_set: too many vectors in one call");
    for (u64 i = 0; i < n; ++i)
        FGPU_REQUIRE(ids[i] < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_vecidx_set: id %llu does not fit (ids are below 2^32 - 1)",
                     (unsigned long long)ids[i]);
    FGPU_REQUIRE(all_finite(vecs, (size_t)n * x->dim), FGPU_INVALID, "fgpu_vecidx_set: a component is NaN or infinite");
    // the slot of every id: the last occurrence of an id is the one written
    std::unordered_map<u32, u32> fresh;   // ids new in this call -> slot
    std::unordered_map<u32, u32> last;    // slot -> row of vecs that wins it
    u32 next = x->count;
    for (u64 i = 0; i < n; ++i) {
        const u32 id = (u32)ids[i];
        u32 s;
        auto it = x->slot_of.find(id);
        if (it != x->slot_of.end()) s = it->second;
        else {
            auto f = fresh.find(id);
            if (f != fresh.end()) s = f->second;
            else {
                FGPU_REQUIRE(next < 0xFFFFFFF0u, FGPU_INVALID, "fgpu_vecidx_set: the store is full");
                s = next++;
                fresh[id] = s;
            }
        }
        last[s] = (u32)i;
    }
    const u64 nwin = last.size();
    std::vector<u32> h(3 * nwin);   // row of vecs, slot, id
    {
        u64 w = 0;
        for (const auto& kv : last) { h[w] = kv.second; h[nwin + w] = kv.first; h[2 * nwin + w] = (u32)ids[kv.second]; ++w; }
    }
    FGPU_TRY(vec_reserve(ctx, x, next));
    hipStream_t st = ctx->stream();
    DevBuf<float> raw;
    DevBuf<u32> d;
    FGPU_TRY(raw.alloc(ctx, (size_t)n * x->dim));
    FGPU_TRY(d.alloc(ctx, 3 * nwin));
    FGPU_TRY(ctx->h2d(raw.p, vecs, (size_t)n * x->dim * sizeof(float)));
    FGPU_TRY(ctx->h2d(d.p, h.data(), 3 * nwin * sizeof(u32)));
    FGPU_TRY(launch(vec_pack_kernel, dim3(grid_for(ctx, nwin * x->nch * 4, 256, 16)), dim3(256), 0, st, (const float*)raw.p,
                    (const u32*)d.p, (const u32*)(d.p + nwin), nwin, x->dim, x->nch, x->store.p));
    FGPU_TRY(launch(vec_norm_kernel, dim3(grid_for(ctx, nwin, 256, 16)), dim3(256), 0, st, (const float*)raw.p, (const u32*)d.p,
                    (const u32*)(d.p + nwin), nwin, x->dim, x->norm.p));
    FGPU_TRY(launch(vec_ids_kernel, dim3(grid_for(ctx, nwin, 256, 16)), dim3(256), 0, st, (const u32*)(d.p + 2 * nwin),
                    (const u32*)(d.p + nwin), nwin, x->ids.p));
    FGPU_HIP(hipStreamSynchronize(st));   // the next search may come from another lane
    x->id_of.resize(next);
    for (const auto& kv : fresh) { x->slot_of[kv.first] = kv.second; x->id_of[kv.second] = kv.first; }
    x->count = next;
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_remove(fgpu_ctx* ctx, fgpu_vecidx* x, const uint64_t* ids, uint64_t n, uint64_t* removed) {
    FGPU_REQUIRE(ctx && x && (n == 0 || ids), FGPU_NULL_POINTER, "fgpu_vecidx_remove: NULL argument");
    if (removed) *removed = 0;
    // The last vector moves into every hole: worked out on the host first, WITHOUT touching the index's maps, which change
    // only once the device has moved the vectors (a failed call leaves the index as it was).  origin[s] = the slot, as of
    // before this call, whose vector ends in slot s: what moves always comes from at or past the new count and lands below
    // it, so one launch moves all.  now_at = the slot of an id this call has moved.
    std::unordered_map<u32, u32> origin, now_at;
    std::unordered_set<u32> dropped;
    u32 count = x->count;
    auto from_slot = [&](u32 s) { auto o = origin.find(s); return o != origin.end() ? o->second : s; };
    for (u64 i = 0; i < n; ++i) {
        if (ids[i] >= 0xFFFFFFFFull) continue;
        const u32 id = (u32)ids[i];
        if (dropped.count(id)) continue;
        u32 s;
        auto m = now_at.find(id);
        if (m != now_at.end()) s = m->second;
        else {
            auto it = x->slot_of.find(id);
            if (it == x->slot_of.end()) continue;
            s = it->second;
        }
        const u32 lastslot = count - 1;
        dropped.insert(id);
        if (s != lastslot) {
            const u32 src = from_slot(lastslot);
            origin[s] = src;
            now_at[x->id_of[src]] = s;
        }
        origin.erase(lastslot);
        --count;
    }
    std::vector<u32> mv;
    for (const auto& kv : origin)
        if (kv.first < count) mv.push_back(kv.second);
    const u32 nm = (u32)mv.size();
    if (nm) {
        for (const auto& kv : origin)
            if (kv.first < count) mv.push_back(kv.first);
        hipStream_t st = ctx->stream();
        DevBuf<u32> d;
        FGPU_TRY(d.alloc(ctx, 2 * (size_t)nm));
        FGPU_TRY(ctx->h2d(d.p, mv.data(), 2 * (size_t)nm * sizeof(u32)));
        FGPU_TRY(launch(vec_move_kernel, dim3(grid_for(ctx, (u64)nm * x->nch * 16, 256, 16)), dim3(256), 0, st, (const u32*)d.p,
                        (const u32*)(d.p + nm), nm, x->nch, x->store.p, x->norm.p, x->ids.p));
        FGPU_HIP(hipStreamSynchronize(st));
    }
    // the device agrees: now the maps
    for (u32 k = 0; k < nm; ++k) {
        const u32 id = x->id_of[mv[k]];   // (sources lie at or past the new count, destinations below it: no entry read here
        x->id_of[mv[nm + k]] = id;        //  was written by this loop)
        x->slot_of[id] = mv[nm + k];
    }
    for (u32 id : dropped) x->slot_of.erase(id);
    x->id_of.resize(count);
    x->count = count;
    if (removed) *removed = dropped.size();
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_get(fgpu_ctx* ctx, const fgpu_vecidx* x, uint64_t id, float* vec, int* present) {
    FGPU_REQUIRE(ctx && x && vec && present, FGPU_NULL_POINTER, "fgpu_vecidx_get: NULL argument");
    *present = 0;
    if (id >= 0xFFFFFFFFull) return FGPU_OK;
    auto it = x->slot_of.find((u32)id);
    if (it == x->slot_of.end()) return FGPU_OK;
    DevBuf<float> out;
    FGPU_TRY(out.alloc(ctx, x->dim));
    FGPU_TRY(launch(vec_get_kernel, dim3((x->dim + 255) / 256), dim3(256), 0, ctx->stream(), (const float*)x->store.p, it->second,
                    x->dim, x->nch, out.p));
    FGPU_TRY(ctx->d2h(vec, out.p, (size_t)x->dim * sizeof(float)));
    *present = 1;
    return FGPU_OK;
}

fgpu_info fgpu_vecidx_knn(fgpu_ctx* ctx, const fgpu_vecidx* x, const float* queries, uint64_t nq, uint64_t k, uint64_t* ids,
                          double* dist, uint64_t* kk_out, uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && x && kk_out && (nq == 0 || queries), FGPU_NULL_POINTER, "fgpu_vecidx_knn: NULL argument");
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    *kk_out = 0;
    FGPU_REQUIRE(k >= 1, FGPU_INVALID, "fgpu_vecidx_knn: k must be at least 1");
    FGPU_REQUIRE(nq < (1ull << 28), FGPU_INVALID, "fgpu_vecidx_knn: too many queries in one call");
    if (nq == 0 || x->count == 0) return FGPU_OK;
    FGPU_REQUIRE(ids && dist, FGPU_NULL_POINTER, "fgpu_vecidx_knn: NULL result array");
    FGPU_REQUIRE(all_finite(queries, (size_t)nq * x->dim), FGPU_INVALID, "fgpu_vecidx_knn: a query component is NaN or infinite");
    const u32 count = x->count, nch = x->nch, dim = x->dim;
    const u32 kk = (u32)std::min<u64>(k, count);
    const u32 ntiles = (count + VT - 1) / VT, stride = ntiles * VT;
    // queries per chunk: 16, 32, or a multiple of 64 whose key images fit the budget, and whose survivors (slot, FP64 distance,
    // u64 id: 20 bytes each, kk per query) fit it too.  Never fewer than one tile of 16.
    u64 qc = std::min<u64>(SCORE_BUDGET / ((size_t)stride * sizeof(u32)), SCORE_BUDGET / ((size_t)kk * 20));
    qc = qc >= 64 ? std::min<u64>((qc / 64) * 64, SEL_QUERIES_MAX) : qc >= 32 ? 32 : 16;
    const u64 nq_pad = nq <= 16 ? 16 : nq <= 32 ? 32 : (nq + 63) / 64 * 64;
    if (qc > nq_pad) qc = nq_pad;
    hipStream_t st = ctx->stream();
    DevBuf<float> raw, qblk, qn;
    DevBuf<u32> scores, hist, out_slot;
    DevBuf<VecSel> sel;
    DevBuf<double> dd;
    DevBuf<u64> did;
    DevBuf<unsigned long long> ties;
    FGPU_TRY(raw.alloc(ctx, (size_t)qc * dim));
    FGPU_TRY(qblk.alloc(ctx, (size_t)qc * nch * 16));
    FGPU_TRY(qn.alloc(ctx, qc));
    FGPU_TRY(scores.alloc(ctx, (size_t)qc * stride));
    FGPU_TRY(hist.alloc(ctx, (size_t)qc * 256));
    FGPU_TRY(sel.alloc(ctx, qc));
    FGPU_TRY(out_slot.alloc(ctx, (size_t)qc * kk));
    FGPU_TRY(dd.alloc(ctx, (size_t)qc * kk));
    FGPU_TRY(did.alloc(ctx, (size_t)qc * kk));
    FGPU_TRY(ties.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(ties.p, 0, sizeof(unsigned long long), st));
    const u32 parts = (count + SEL_PER_WG - 1) / SEL_PER_WG;
    u64 launches = 0, qtiles = 0, bytes = 0;
    for (u64 q0 = 0; q0 < nq; q0 += qc) {
        const u32 m = (u32)std::min<u64>(qc, nq - q0);               // real queries of this chunk
        const u32 mp = m <= 16 ? 16 : m <= 32 ? 32 : (m + 63) / 64 * 64;   // ... padded to what one kernel form serves
        const int nqt = mp == 16 ? 1 : mp == 32 ? 2 : 4;
        FGPU_TRY(ctx->h2d(raw.p, queries + (size_t)q0 * dim, (size_t)m * dim * sizeof(float)));
        FGPU_HIP(hipMemsetAsync(qblk.p, 0, (size_t)mp * nch * 16 * sizeof(float), st));
        FGPU_HIP(hipMemsetAsync(qn.p, 0, (size_t)mp * sizeof(float), st));
        FGPU_TRY(launch(vec_pack_kernel, dim3(grid_for(ctx, (u64)m * nch * 4, 256, 16)), dim3(256), 0, st, (const float*)raw.p,
                        nullptr, nullptr, (u64)m, dim, nch, qblk.p));
        FGPU_TRY(launch(vec_norm_kernel, dim3(grid_for(ctx, m, 256, 16)), dim3(256), 0, st, (const float*)raw.p, nullptr, nullptr,
                        (u64)m, dim, qn.p));
        const u32 groups = mp / 16 / nqt;
        {
            ProfScope ps(ctx, "vec_score", (u64)groups * ntiles * nch * 1024);
            const dim3 grid(grid_for(ctx, ntiles, 4, 8), groups);
            auto score = [&](auto c) {
                return launch(vec_score_kernel<decltype(c)::value>, grid, dim3(256), 0, st, (const float4*)x->store.p,
                              (const float4*)qblk.p, (const float*)x->norm.p, (const float*)qn.p, scores.p, ntiles, nch, stride,
                              x->metric);
            };
            const fgpu_info si = pick<1, 2, 4>(nqt, score);
            FGPU_TRY(si);
        }
        ++launches;
        qtiles += mp / 16;
        bytes += (u64)groups * ntiles * nch * 1024;
        const u64 total = (u64)m * kk;
        {
            ProfScope ps(ctx, "vec_select", (u64)m * count * sizeof(u32));
            FGPU_TRY(launch(vec_sel_init_kernel, dim3((m * 256 + 255) / 256), dim3(256), 0, st, sel.p, hist.p, m, kk));
            for (int shift = 56; shift >= 0; shift -= 8) {
                FGPU_TRY(launch(vec_sel_hist_kernel, dim3(parts, m), dim3(256), 0, st, (const u32*)scores.p, (const u32*)x->ids.p,
                                (const VecSel*)sel.p, hist.p, count, stride, (u32)shift));
                FGPU_TRY(launch(vec_sel_pick_kernel, dim3(m), dim3(256), 0, st, sel.p, hist.p, (u32)shift));
            }
            FGPU_TRY(launch(vec_sel_compact_kernel, dim3(parts, m), dim3(256), 0, st, (const u32*)scores.p, (const u32*)x->ids.p,
                            sel.p, count, stride, kk, out_slot.p, ties.p));
        }
        {
            ProfScope ps(ctx, "vec_dist", total * nch * 64);
            FGPU_TRY(launch(vec_dist_kernel, dim3(grid_for(ctx, total, 256, 16)), dim3(256), 0, st, (const float*)x->store.p,
                            (const float*)qblk.p, (const u32*)x->ids.p, (const u32*)out_slot.p, total, kk, nch, x->metric, dd.p,
                            did.p));
        }
        {
            ProfScope ps(ctx, "vec_readback", total * (sizeof(double) + sizeof(u64)));
            FGPU_TRY(ctx->d2h(dist + (size_t)q0 * kk, dd.p, total * sizeof(double)));
            FGPU_TRY(ctx->d2h(ids + (size_t)q0 * kk, did.p, total * sizeof(u64)));
        }
    }
    unsigned long long tie_total = 0;
    if (stats) FGPU_TRY(ctx->d2h(&tie_total, ties.p, sizeof(tie_total)));
    FGPU_HIP(hipStreamSynchronize(st));
    // ascending (D, id) per query
    std::vector<std::pair<double, u64>> row(kk);
    for (u64 q = 0; q < nq; ++q) {
        double* dr = dist + (size_t)q * kk;
        u64* ir = ids + (size_t)q * kk;
        for (u32 j = 0; j < kk; ++j) row[j] = {dr[j], ir[j]};
        std::sort(row.begin(), row.end());
        for (u32 j = 0; j < kk; ++j) { dr[j] = row[j].first; ir[j] = row[j].second; }
    }
    *kk_out = kk;
    if (stats) { stats[0] = launches; stats[1] = qtiles; stats[2] = bytes; stats[3] = tie_total; }
    return FGPU_OK;
}

}  // extern "C"
