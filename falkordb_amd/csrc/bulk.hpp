// bulk.hpp — the prelude of the bulk mutations: fgpu_edges_build (edges.hip), fgpu_nodes_detach (detach.hip), fgpu_edges_remove
// (edges_remove.hip) and fgpu_edges_union (edges_union.hip) open and close with the same steps, and the next mutation calls them
// instead of copying them.  merge.hip shares the row searches and the wordrow kernel.
//
//   searches  lower_bound over a sorted range of positions, and what the mutations build on it: find, probe / locate of a pair
//             in a snapshot, row_begin, and row_of over row pointers.  Positions reach 2^32 - 2, so every midpoint is
//             lo + (hi - lo) / 2: the sum lo + hi wraps once a range lies past 2^31
//   count_if  a counter that places nothing: a ballot and one atomicAdd per wavefront
//   wordrow   the stored row of every 64th entry, a lane per word: entry_row searches the row pointers between wordrow[p / 64]
//             and wordrow[p / 64 + 1] only.  The bulk entry points build theirs per call (wordrow_build) and keep it off the
//             snapshot: a rejected call must leave no device memory on the caller's inputs
//   host      marshal_triples and MultiRows check the caller's arrays and narrow them to the 32-bit id space, in the order the
//             entry points always checked them; require_pattern_of; published() closes an extern "C" entry
//
// Everything is static or inline: each translation unit carries its own copy.
#pragma once
#include <vector>

#include "common.hpp"

namespace fgpu {

// ---- searches -----------------------------------------------------------------------------------------------------------
// first position in [b, e) of the ascending a whose element is not below x, or e
template <typename T>
__device__ __forceinline__ u32 lower_bound(const T* __restrict__ a, u32 b, u32 e, T x) {
    u32 lo = b, hi = e;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// position of x in [b, e) of the ascending a, or ~0u
template <typename T>
__device__ __forceinline__ u32 find(const T* __restrict__ a, u32 b, u32 e, T x) {
    const u32 lo = lower_bound(a, b, e, x);
    return (lo < e && a[lo] == x) ? lo : ~0u;
}
// position of the entry (r, c) of a, or ~0u
__device__ __forceinline__ u32 probe(const CsrView& a, u32 r, u32 c) {
    u32 b, e;
    row_range(a, r, b, e);
    return find(a.colidx, b, e, c);
}
// first entry of the first stored row at or past r (r <= nrows)
__device__ __forceinline__ u32 row_begin(const CsrView& a, u32 r) {
    return a.rowptr[a.hrows ? lower_bound(a.hrows, 0u, a.nvec, r) : r];
}
// the entry (r, c) of a, or the position it would be inserted at (r < nrows)
__device__ __forceinline__ u32 locate(const CsrView& a, u32 r, u32 c, bool& found) {
    u32 i = r;
    if (a.hrows) {
        i = lower_bound(a.hrows, 0u, a.nvec, r);
        if (i == a.nvec || a.hrows[i] != r) { found = false; return a.rowptr[i]; }
    }
    const u32 e = a.rowptr[i + 1], lo = lower_bound(a.colidx, a.rowptr[i], e, c);
    found = lo < e && a.colidx[lo] == c;
    return lo;
}
// largest i in [lo, hi] with rp[i] <= p (rows may be empty: equal row pointers); the midpoint is the upper one, lo + ceil((hi - lo) / 2)
__device__ __forceinline__ u32 row_of(const u32* __restrict__ rp, u32 lo, u32 hi, u32 p) {
    while (lo < hi) {
        const u32 mid = hi - ((hi - lo) >> 1);
        if (rp[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// *counter += the lanes of the wavefront whose flag is set (every lane of the wavefront calls it)
__device__ __forceinline__ void count_if(bool flag, u32* __restrict__ counter) {
    const u64 b = __ballot(flag);
    if (lane_id() == 0 && b) atomicAdd(counter, (u32)__popcll(b));
}

// ---- the wordrow index --------------------------------------------------------------------------------------------------
// stored-row index of the first entry of each 64-entry word; wordrow[nwords] = last stored row
static __global__ __launch_bounds__(256) void wordrow_kernel(const u32* __restrict__ rp, u32 nvec, u32 nwords,
                                                            u32* __restrict__ wordrow) {
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w > nwords) return;
    wordrow[w] = w < nwords ? row_of(rp, 0, nvec - 1, w << 6) : nvec - 1;
}
// the stored row of entry p, and its row id
__device__ __forceinline__ u32 entry_vec(const u32* __restrict__ rp, const u32* __restrict__ wordrow, u32 p) {
    const u32 w = p >> 6;
    return row_of(rp, wordrow[w], wordrow[w + 1], p);
}
__device__ __forceinline__ u32 entry_row(const CsrView& a, const u32* __restrict__ wordrow, u32 p) {
    const u32 i = entry_vec(a.rowptr, wordrow, p);
    return a.hrows ? a.hrows[i] : i;
}
// out = the wordrow index of the n > 0 entries that the nvec + 1 row pointers rp divide
static fgpu_info wordrow_build(fgpu_ctx* ctx, const u32* rp, u32 nvec, u64 n, DevBuf<u32>& out) {
    const u32 nwords = (u32)((n + 63) >> 6);
    FGPU_TRY(out.alloc(ctx, (size_t)nwords + 1));
    return launch(wordrow_kernel, dim3(cdiv((u64)nwords + 1, 256)), dim3(256), 0, ctx->stream(), rp, nvec, nwords, out.p);
}

// ---- host: the caller's arrays ------------------------------------------------------------------------------------------
// n (src, dst, id) triples of fn: each inside nrows x ncols and its id not the marker, the coordinates narrowed into s32 / d32
static fgpu_info marshal_triples(const char* fn, const u64* srcs, const u64* dsts, const u64* ids, u64 n, u64 nrows, u64 ncols,
                                 std::vector<u32>& s32, std::vector<u32>& d32) {
    s32.resize(n);
    d32.resize(n);
    for (u64 k = 0; k < n; ++k) {
        FGPU_REQUIRE(srcs[k] < nrows && dsts[k] < ncols, FGPU_INVALID, "%s: triple %llu = (%llu, %llu) outside %llu x %llu", fn,
                     (unsigned long long)k, (unsigned long long)srcs[k], (unsigned long long)dsts[k], (unsigned long long)nrows,
                     (unsigned long long)ncols);
        FGPU_REQUIRE(ids[k] != FGPU_MULTI_EDGE, FGPU_INVALID, "%s: triple %llu carries the MULTI_EDGE marker as its id", fn,
                     (unsigned long long)k);
        s32[k] = (u32)srcs[k];
        d32[k] = (u32)dsts[k];
    }
    return FGPU_OK;
}

// supplied multi-edge rows (key = src << 32 | dst ascending, ids of row r = ids[off[r], off[r + 1]) ascending, at least 2 of
// them): checked and the offsets narrowed to 32 bits by check(), on the device after upload()
struct MultiRows {
    const u64 *key_h = nullptr, *ids_h = nullptr;
    u64 n = 0;
    std::vector<u32> off32;
    DevBuf<u64> key, ids;
    DevBuf<u32> off;

    u64 total() const { return off32[n]; }   // ids in all rows
    fgpu_info check(const char* fn, const char* what, const u64* key_in, const u64* off_in, const u64* ids_in, u64 n_in) {
        key_h = key_in;
        ids_h = ids_in;
        n = n_in;
        off32.assign((size_t)n + 1, 0u);
        FGPU_REQUIRE(n == 0 || off_in[0] == 0, FGPU_INVALID, "%s: %s_off[0] is not 0", fn, what);
        for (u64 r = 0; r < n; ++r) {
            FGPU_REQUIRE(r == 0 || key_h[r - 1] < key_h[r], FGPU_INVALID, "%s: %s key %llu is not above the one before it", fn, what,
                         (unsigned long long)r);
            const u64 b = off_in[r], e = off_in[r + 1];
            FGPU_REQUIRE(e >= b + 2 && e < 0xFFFFFFFFull, FGPU_INVALID, "%s: %s row %llu holds fewer than 2 ids (offsets %llu, %llu)", fn,
                         what, (unsigned long long)r, (unsigned long long)b, (unsigned long long)e);
            for (u64 j = b + 1; j < e; ++j)
                FGPU_REQUIRE(ids_h[j - 1] < ids_h[j], FGPU_INVALID, "%s: the ids of %s row %llu do not ascend", fn, what,
                             (unsigned long long)r);
            FGPU_REQUIRE(ids_h[e - 1] != FGPU_MULTI_EDGE, FGPU_INVALID, "%s: %s row %llu carries the MULTI_EDGE marker as an id", fn, what,
                         (unsigned long long)r);
            off32[r + 1] = (u32)e;
        }
        return FGPU_OK;
    }
    fgpu_info upload(fgpu_ctx* ctx, const char* prof_name) {   // (prof_name: a static string)
        const u64 T = total();
        FGPU_TRY(key.alloc(ctx, n));
        FGPU_TRY(off.alloc(ctx, n + 1));
        FGPU_TRY(ids.alloc(ctx, T));
        ProfScope prof(ctx, prof_name, n * 12 + T * 8);
        FGPU_TRY(ctx->h2d(off.p, off32.data(), (n + 1) * sizeof(u32)));
        if (n) {
            FGPU_TRY(ctx->h2d(key.p, key_h, n * sizeof(u64)));
            FGPU_TRY(ctx->h2d(ids.p, ids_h, T * sizeof(u64)));
        }
        return FGPU_OK;
    }
};

// t (called `what` in fn's messages) is the BOOL pattern of m's transposed shape
static fgpu_info require_pattern_of(const char* fn, const char* what, const fgpu_mat* t, const fgpu_mat* m) {
    FGPU_REQUIRE(t, FGPU_INVALID, "%s: the transposed pattern %s is missing", fn, what);
    FGPU_REQUIRE(t->nrows == m->ncols && t->ncols == m->nrows && !t->vals, FGPU_INVALID,
                 "%s: %s must be the BOOL %llu x %llu pattern (got %llu x %llu%s)", fn, what, (unsigned long long)m->ncols,
                 (unsigned long long)m->nrows, (unsigned long long)t->nrows, (unsigned long long)t->ncols, t->vals ? ", valued" : "");
    return FGPU_OK;
}

// the tail of an extern "C" producer of snapshots: the new handles may go to another thread
inline fgpu_info published(fgpu_ctx* ctx, fgpu_info info) { return (info == FGPU_OK && ctx) ? ctx->publish() : info; }

}  // namespace fgpu
