// edges.hip — fgpu_edges_build: one relationship type's bulk batch of (src, dst, edge id) tuples -> what a Tensor holds for it
// (tensor.rs:184-205; the per-pair states of tensor.rs:72-108): the UINT64 forward matrix with the edge id inline for a pair
// with one edge and MULTI_EDGE for a pair with several, the BOOL transposed pattern, and every multi-edge pair's ids ascending.
// The reference feeds Graph::create_relationships_bulk one type at a time (graph.rs:2062-2121) and folds afterwards
// (flush_for_bulk, :2129-2140); this is that result for an empty tensor, built in one call.
//
//   sort    the tuple INDICES ordered by (src, dst, input position): two passes of the stable counting sort of transpose.hip
//           (by dst, then by src of the permuted order) — below 4096 tuples one workgroup sorts (pair, position) in LDS, and a
//           dimension past 2^31 goes through the same stable sort in 16-bit digits.  Every later stage sees one permutation.
//   runs    a lane per sorted position: head = "pair differs from the predecessor"; three exclusive scans give every head its
//           entry of the forward matrix, every multi-edge head its run index and every id of a multi-edge run its slot.  One
//           pass writes colidx / vals, the run keys, offsets and ids (input order: the sort is stable), and compares every id
//           with its run predecessor: equal = the same (src, dst, id) twice, smaller = the run arrived out of order.  The row
//           pointers are a lane per row: a binary search for the row's first sorted position.
//   order   the runs that arrived out of order are listed (a scan) and sorted by segsort_u64 (prims.hip); those longer than 4096
//           ids are sorted by the host after the read-back.  Freshly allocated ascending ids sort nothing.
//   bwd     the pattern transpose of the forward matrix (mat_transpose_pattern).
//
// No wavefront per row and no atomics anywhere: every list is placed by a scan, the flags are plain stores of 1.
#include <algorithm>

#include "bulk.hpp"

namespace fgpu {

constexpr u64 EB_SMALL_MAX = 4096;    // fewer tuples than this are sorted by one workgroup in LDS
constexpr u64 EB_HOST_RUN = 4096;     // runs longer than this that arrived out of order are sorted by the host

// ---- sort -------------------------------------------------------------------------------------------------------------
// (pair, position) of up to 4095 tuples, bitonic in LDS: position breaks ties, so the order is the stable one
__global__ __launch_bounds__(256) void eb_small_sort_kernel(const u32* __restrict__ src, const u32* __restrict__ dst, u32 n,
                                                           u32* __restrict__ perm) {
    __shared__ u64 s_key[EB_SMALL_MAX];
    __shared__ u32 s_idx[EB_SMALL_MAX];
    u32 p2 = 2;
    while (p2 < n) p2 <<= 1;
    for (u32 i = threadIdx.x; i < p2; i += 256) {
        s_key[i] = i < n ? ((u64)src[i] << 32) | dst[i] : ~0ull;   // (no pair is ~0: dimensions stop below 2^32 - 1)
        s_idx[i] = i;
    }
    __syncthreads();
    for (u32 k = 2; k <= p2; k <<= 1) {
        for (u32 j = k >> 1; j >= 1; j >>= 1) {
            for (u32 t = threadIdx.x; t < (p2 >> 1); t += 256) {
                const u32 i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const u32 l = i | j;
                const u64 a = s_key[i], c = s_key[l];
                const u32 ai = s_idx[i], ci = s_idx[l];
                const bool gt = a > c || (a == c && ai > ci);
                const bool up = ((i & k) == 0);
                if (gt == up) { s_key[i] = c; s_key[l] = a; s_idx[i] = ci; s_idx[l] = ai; }
            }
            __syncthreads();
        }
    }
    for (u32 i = threadIdx.x; i < n; i += 256) perm[i] = s_idx[i];
}

__global__ __launch_bounds__(256) void eb_iota_kernel(u32* __restrict__ v, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = (u32)i;
}

// the next pass's keys: a digit of the coordinate of the tuple at every position of the order so far
__global__ __launch_bounds__(256) void eb_digit_kernel(const u32* __restrict__ coord, const u32* __restrict__ perm, u64 n,
                                                      u32 shift, u32 mask, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (coord[perm[i]] >> shift) & mask;
}

// one stable pass: perm_out = perm_in reordered by coord[perm_in[.]] (< nkeys)
static fgpu_info eb_sort_pass(fgpu_ctx* ctx, const u32* coord, const u32* perm_in, u64 n, u64 nkeys, u32* keys, u32* perm_out,
                              bool* by_digits) {
    hipStream_t st = ctx->stream();
    const dim3 grid(cdiv(n, 256));
    FGPU_TRY(launch(eb_digit_kernel, grid, dim3(256), 0, st, coord, perm_in, n, 0u, 0xFFFFFFFFu, keys));
    DevBuf<u32> keyptr;
    if (nkeys <= (1ull << 31)) {
        FGPU_TRY(keyptr.alloc(ctx, nkeys + 1));
        const fgpu_info i = sort_u32_pairs_stable(ctx, keys, perm_in, n, nkeys, perm_out, keyptr.p);
        if (i != FGPU_NO_VALUE) return i;
    }
    // a key space past 2^31: the same stable sort, least significant 16 bits first
    *by_digits = true;
    FGPU_TRY(keyptr.alloc(ctx, 65536 + 1));
    DevBuf<u32> mid;
    FGPU_TRY(mid.alloc(ctx, n));
    FGPU_TRY(launch(eb_digit_kernel, grid, dim3(256), 0, st, coord, perm_in, n, 0u, 0xFFFFu, keys));
    FGPU_TRY(sort_u32_pairs_by_key(ctx, keys, perm_in, n, 65536, mid.p, keyptr.p));
    FGPU_TRY(launch(eb_digit_kernel, grid, dim3(256), 0, st, coord, (const u32*)mid.p, n, 16u, 0xFFFFu, keys));
    FGPU_TRY(sort_u32_pairs_by_key(ctx, keys, mid.p, n, 65536, perm_out, keyptr.p));
    return FGPU_OK;
}

// ---- runs -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eb_sorted_kernel(const u32* __restrict__ src, const u32* __restrict__ dst,
                                                       const u64* __restrict__ ids, const u32* __restrict__ perm, u64 n,
                                                       u64* __restrict__ key, u64* __restrict__ sid) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 t = perm[i];
    key[i] = ((u64)src[t] << 32) | dst[t];
    sid[i] = ids[t];
}

// head: first tuple of its pair; mhead: head of a pair with several tuples; inm: tuple of such a pair
__global__ __launch_bounds__(256) void eb_flag_kernel(const u64* __restrict__ key, u64 n, u32* __restrict__ head,
                                                     u32* __restrict__ mhead, u32* __restrict__ inm) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const bool h = i == 0 || key[i - 1] != k;
    const bool last = i + 1 == n || key[i + 1] != k;
    head[i] = h ? 1u : 0u;
    mhead[i] = (h && !last) ? 1u : 0u;
    inm[i] = (h && last) ? 0u : 1u;
}

// E / R / P: the exclusive scans of head / mhead / inm
__global__ __launch_bounds__(256) void eb_emit_kernel(const u64* __restrict__ key, const u64* __restrict__ sid,
                                                     const u32* __restrict__ E, const u32* __restrict__ R,
                                                     const u32* __restrict__ P, u64 n, u32 n_multi, u32 n_mids,
                                                     u32* __restrict__ colidx, u64* __restrict__ vals, u64* __restrict__ mkey,
                                                     u32* __restrict__ moff, u64* __restrict__ mids, u32* __restrict__ unsorted,
                                                     u32* __restrict__ dup_flag) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) moff[n_multi] = n_mids;
    const u64 k = key[i], id = sid[i];
    const bool h = i == 0 || key[i - 1] != k;
    const bool last = i + 1 == n || key[i + 1] != k;
    if (h) {
        const u32 e = E[i];
        colidx[e] = (u32)k;
        vals[e] = last ? id : ~0ull;
    }
    if (h && last) return;
    const u32 p = P[i];
    mids[p] = id;
    if (h) {
        const u32 r = R[i];
        mkey[r] = k;
        moff[r] = p;
    } else {
        const u64 prev = sid[i - 1];
        if (id == prev) *dup_flag = 1u;
        else if (id < prev) unsorted[R[i] - 1u] = 1u;   // (the run's head lies before i: R[i] counts it)
    }
}

// rowptr[r] = entries before row r: the entry of the first sorted position whose source is >= r
__global__ __launch_bounds__(256) void eb_rowptr_kernel(const u64* __restrict__ key, u64 n, const u32* __restrict__ E,
                                                       u32 n_distinct, u64 nrows, u32* __restrict__ rowptr) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    const u32 lo = lower_bound(key, 0u, (u32)n, r << 32);
    rowptr[r] = lo < n ? E[lo] : n_distinct;
}

__global__ __launch_bounds__(256) void eb_ulist_kernel(const u32* __restrict__ unsorted, const u32* __restrict__ upos,
                                                      u32 n_multi, u32* __restrict__ ulist) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r < n_multi && unsorted[r]) ulist[upos[r]] = r;
}

static fgpu_info eb_empty(fgpu_ctx* ctx, fgpu_mat** out, u64 nrows, u64 ncols, bool with_vals) {
    MatRef m;
    FGPU_TRY(mat_alloc(ctx, &m.m, nrows, ncols, 0, with_vals, 0, true));
    FGPU_HIP(hipMemsetAsync(m->rowptr, 0, sizeof(u32), ctx->stream()));
    FGPU_TRY(mat_finalize(m.get()));
    *out = m.release();
    return FGPU_OK;
}

static fgpu_info edges_build_impl(fgpu_ctx* ctx, u64 nrows, u64 ncols, const u64* srcs, const u64* dsts, const u64* ids, u64 n,
                                  fgpu_mat** fwd_out, fgpu_mat** bwd_out, u64** multi_key, u64** multi_off, u64** multi_ids,
                                  u64* n_multi_out, u64* stats) {
    FGPU_REQUIRE(ctx && fwd_out && bwd_out && multi_key && multi_off && multi_ids && n_multi_out, FGPU_NULL_POINTER,
                 "fgpu_edges_build: NULL argument");
    FGPU_REQUIRE(n == 0 || (srcs && dsts && ids), FGPU_NULL_POINTER, "fgpu_edges_build: NULL tuple arrays");
    *fwd_out = *bwd_out = nullptr;
    *multi_key = *multi_off = *multi_ids = nullptr;
    *n_multi_out = 0;
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(nrows < 0xFFFFFFFFull && ncols < 0xFFFFFFFFull, FGPU_INVALID,
                 "fgpu_edges_build: dims %llu x %llu exceed the 32-bit id space", (unsigned long long)nrows,
                 (unsigned long long)ncols);
    FGPU_REQUIRE(n < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_edges_build: %llu tuples exceed the 32-bit position space",
                 (unsigned long long)n);
    hipStream_t st = ctx->stream();
    MatRef fwd, bwd;
    ResultBuf rk, ro, ri;
    u64 n_multi = 0, n_mids = 0, n_distinct = 0, n_unsorted = 0, n_host_sorted = 0, longest = 0, path = 0;
    if (n == 0) {
        FGPU_TRY(eb_empty(ctx, &fwd.m, nrows, ncols, true));
        FGPU_TRY(eb_empty(ctx, &bwd.m, ncols, nrows, false));
        FGPU_REQUIRE(ro.alloc_host(ctx, sizeof(u64)), FGPU_OOM, "fgpu_edges_build: out of host memory");
        *(u64*)ro.p = 0;
    } else {
        // ---- marshal + upload ------------------------------------------------------------------------------------
        DevBuf<u32> dsrc, ddst;
        DevBuf<u64> dids;
        {
            std::vector<u32> s32, d32;
            FGPU_TRY(marshal_triples("fgpu_edges_build", srcs, dsts, ids, n, nrows, ncols, s32, d32));
            ProfScope ps(ctx, "eb_h2d", 16 * n);
            FGPU_TRY(dsrc.alloc(ctx, n));
            FGPU_TRY(ddst.alloc(ctx, n));
            FGPU_TRY(dids.alloc(ctx, n));
            FGPU_TRY(ctx->h2d(dsrc.p, s32.data(), n * sizeof(u32)));
            FGPU_TRY(ctx->h2d(ddst.p, d32.data(), n * sizeof(u32)));
            FGPU_TRY(ctx->h2d(dids.p, ids, n * sizeof(u64)));
        }
        const dim3 grid(cdiv(n, 256));
        // ---- sort -------------------------------------------------------------------------------------------------
        DevBuf<u32> perm;
        FGPU_TRY(perm.alloc(ctx, n));
        {
            ProfScope ps(ctx, "eb_sort", 0);
            if (n < EB_SMALL_MAX) {
                FGPU_TRY(launch(eb_small_sort_kernel, dim3(1), dim3(256), 0, st, (const u32*)dsrc.p, (const u32*)ddst.p, (u32)n, perm.p));
            } else {
                DevBuf<u32> iota, keys, perm1;
                FGPU_TRY(iota.alloc(ctx, n));
                FGPU_TRY(keys.alloc(ctx, n));
                FGPU_TRY(perm1.alloc(ctx, n));
                FGPU_TRY(launch(eb_iota_kernel, grid, dim3(256), 0, st, iota.p, n));
                bool digits = false;
                FGPU_TRY(eb_sort_pass(ctx, ddst.p, iota.p, n, ncols, keys.p, perm1.p, &digits));
                FGPU_TRY(eb_sort_pass(ctx, dsrc.p, perm1.p, n, nrows, keys.p, perm.p, &digits));
                path = digits ? 2 : 1;
            }
        }
        // ---- runs -------------------------------------------------------------------------------------------------
        DevBuf<u64> key, sid, dmkey, dmids;
        DevBuf<u32> E, R, P, tot, dmoff, unsorted;
        {
            ProfScope ps(ctx, "eb_runs", 0);
            FGPU_TRY(key.alloc(ctx, n));
            FGPU_TRY(sid.alloc(ctx, n));
            FGPU_TRY(launch(eb_sorted_kernel, grid, dim3(256), 0, st, (const u32*)dsrc.p, (const u32*)ddst.p, (const u64*)dids.p,
                            (const u32*)perm.p, n, key.p, sid.p));
            perm.release(); dsrc.release(); ddst.release(); dids.release();
            FGPU_TRY(E.alloc(ctx, n));
            FGPU_TRY(R.alloc(ctx, n));
            FGPU_TRY(P.alloc(ctx, n));
            FGPU_TRY(tot.alloc(ctx, 8));   // [0] pairs [1] multi pairs [2] ids of multi pairs [3] runs out of order [4] duplicate triple
            FGPU_HIP(hipMemsetAsync(tot.p, 0, 8 * sizeof(u32), st));
            FGPU_TRY(launch(eb_flag_kernel, grid, dim3(256), 0, st, (const u64*)key.p, n, E.p, R.p, P.p));
            FGPU_TRY(scan_u32(ctx, E.p, E.p, n, tot.p + 0));
            FGPU_TRY(scan_u32(ctx, R.p, R.p, n, tot.p + 1));
            FGPU_TRY(scan_u32(ctx, P.p, P.p, n, tot.p + 2));
            u32 h[3];
            FGPU_TRY(read_words(ctx, tot.p, 3, h));
            n_distinct = h[0]; n_multi = h[1]; n_mids = h[2];
            FGPU_TRY(mat_alloc(ctx, &fwd.m, nrows, ncols, n_distinct, true, 0, false));
            FGPU_TRY(dmkey.alloc(ctx, n_multi));
            FGPU_TRY(dmoff.alloc(ctx, n_multi + 1));
            FGPU_TRY(dmids.alloc(ctx, n_mids));
            FGPU_TRY(unsorted.alloc(ctx, n_multi));
            FGPU_HIP(hipMemsetAsync(unsorted.p, 0, (n_multi ? n_multi : 1) * sizeof(u32), st));
            FGPU_TRY(launch(eb_emit_kernel, grid, dim3(256), 0, st, (const u64*)key.p, (const u64*)sid.p, (const u32*)E.p,
                            (const u32*)R.p, (const u32*)P.p, n, (u32)n_multi, (u32)n_mids, fwd->colidx, fwd->vals, dmkey.p, dmoff.p,
                            dmids.p, unsorted.p, tot.p + 4));
            FGPU_TRY(launch(eb_rowptr_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, st, (const u64*)key.p, n, (const u32*)E.p,
                            (u32)n_distinct, nrows, fwd->rowptr));
        }
        // ---- the runs that arrived out of order ---------------------------------------------------------------------
        {
            ProfScope ps(ctx, "eb_order", 0);
            DevBuf<u32> upos, ulist;
            if (n_multi) {
                FGPU_TRY(upos.alloc(ctx, n_multi));
                FGPU_TRY(scan_u32(ctx, unsorted.p, upos.p, n_multi, tot.p + 3));
            }
            u32 h[2];
            FGPU_TRY(read_words(ctx, tot.p + 3, 2, h));
            n_unsorted = h[0];
            FGPU_REQUIRE(h[1] == 0, FGPU_INVALID, "fgpu_edges_build: the same (src, dst, id) triple occurs twice");
            if (n_unsorted) {
                FGPU_TRY(ulist.alloc(ctx, n_unsorted));
                FGPU_TRY(launch(eb_ulist_kernel, dim3(cdiv(n_multi, 256)), dim3(256), 0, st, (const u32*)unsorted.p, (const u32*)upos.p,
                                (u32)n_multi, ulist.p));
                FGPU_TRY(segsort_u64(ctx, dmids.p, dmoff.p, ulist.p, (u32)n_unsorted, tot.p + 4));
                u32 dup = 0;
                FGPU_TRY(read_u32(ctx, tot.p + 4, &dup));
                FGPU_REQUIRE(dup == 0, FGPU_INVALID, "fgpu_edges_build: the same (src, dst, id) triple occurs twice");
            }
        }
        key.release(); sid.release(); E.release(); R.release(); P.release();
        // ---- backward pattern ---------------------------------------------------------------------------------------
        {
            ProfScope ps(ctx, "eb_transpose", 0);
            FGPU_TRY(mat_transpose_pattern(ctx, &bwd.m, fwd.get()));
        }
        // ---- read-back ----------------------------------------------------------------------------------------------
        {
            ProfScope ps(ctx, "eb_readback", 16 * n_multi + 8 * n_mids);
            FGPU_REQUIRE(ro.alloc(ctx, (n_multi + 1) * sizeof(u64)), FGPU_OOM, "fgpu_edges_build: out of host memory");
            FGPU_TRY(ctx->d2h_widen((u64*)ro.p, dmoff.p, n_multi + 1));
            if (n_multi) {
                FGPU_REQUIRE(rk.alloc(ctx, n_multi * sizeof(u64)) && ri.alloc(ctx, n_mids * sizeof(u64)), FGPU_OOM,
                             "fgpu_edges_build: out of host memory");
                FGPU_TRY(ctx->d2h(rk.p, dmkey.p, n_multi * sizeof(u64)));
                FGPU_TRY(ctx->d2h(ri.p, dmids.p, n_mids * sizeof(u64)));
            }
        }
        // the long runs: sorted here when they arrived out of order
        const u64* off = (const u64*)ro.p;
        u64* hid = (u64*)ri.p;
        longest = n_distinct ? 1 : 0;
        for (u64 r = 0; r < n_multi; ++r) {
            const u64 b = off[r], e = off[r + 1];
            longest = std::max(longest, e - b);
            if (e - b <= EB_HOST_RUN || std::is_sorted(hid + b, hid + e)) continue;
            std::sort(hid + b, hid + e);
            ++n_host_sorted;
            FGPU_REQUIRE(std::adjacent_find(hid + b, hid + e) == hid + e, FGPU_INVALID,
                         "fgpu_edges_build: the same (src, dst, id) triple occurs twice");
        }
    }
    if (stats) {
        stats[0] = n_distinct;
        stats[1] = n_multi;
        stats[2] = n_mids;
        stats[3] = longest;
        stats[4] = n_unsorted;
        stats[5] = n_unsorted - n_host_sorted;
        stats[6] = n_host_sorted;
        stats[7] = path;
    }
    *fwd_out = fwd.release();
    *bwd_out = bwd.release();
    *multi_key = (u64*)rk.release();
    *multi_off = (u64*)ro.release();
    *multi_ids = (u64*)ri.release();
    *n_multi_out = n_multi;
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_edges_build(fgpu_ctx* ctx, uint64_t nrows, uint64_t ncols, const uint64_t* srcs, const uint64_t* dsts,
                                      const uint64_t* ids, uint64_t n, fgpu_mat** fwd, fgpu_mat** bwd, uint64_t** multi_key,
                                      uint64_t** multi_off, uint64_t** multi_ids, uint64_t* n_multi, uint64_t stats[8]) {
    return published(ctx, edges_build_impl(ctx, nrows, ncols, srcs, dsts, ids, n, fwd, bwd, multi_key, multi_off, multi_ids, n_multi,
                                           stats));
}
