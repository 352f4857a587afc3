// detach.hip — fgpu_nodes_detach: a set D of nodes leaves a matrix, and its entries go with it (DETACH DELETE).  The reference
// does this on every commit with deleted nodes: Graph::delete_nodes (graph.rs:1698-1772) clears the rows of the node x label
// matrix, Graph::delete_implicit_edges (graph.rs:2386-2494) walks, per relationship type and per deleted node, the node's row of
// the tensor and its row of the transpose, removes what it found with Tensor::remove_all and returns the (edge id, src, dst) list.
// Here one call gives the compacted matrix, the compacted transposed pattern and the removal list in the reference's order:
//
//   bitmap  D as one bit per node (the only atomics of the file: atomicOr into the bitmap, and three counters that place nothing)
//   flags   a lane per ENTRY POSITION p of the matrix: its stored row from a search between wordrow[p / 64] and wordrow[p / 64 + 1]
//           (the row of every 64th entry, a lane per word), keep = "neither end in D" under `sides`, out = "row in D"
//   scans   E = exclusive scan of keep, O = of out, both over nnz + 1 flags, so that E[nnz] and O[nnz] are the totals
//   emit    kept entry p -> position E[p] of the output; out entry p -> position O[p] of the list.  Positions ascend with p and
//           p ascends in (row, col): the list is in ascending (src, dst) without a sort
//   rows    rowptr'[r] = E[rowptr[r]], a lane per row — no per-row loop; a hypersparse input goes through its hrows, and the
//           output is hypersparse exactly when fgpu_mat_from_coo would store that many populated rows so (prefer_hyper)
//   mt      the same four steps over the transposed pattern, rows and columns swapped, with the list flag in = "row in D and
//           column not": the scan orders the in-list in ascending (dst, src), the order a walk of mt's rows meets them.  Each in
//           entry takes its value by a binary search for dst in row src of the forward matrix
//
// No wavefront per row anywhere: a hub row of 10^6 entries is 10^6 lanes like any other 10^6 entries.  The emit and rows steps
// live in compact.hpp, which fgpu_edges_remove (edges_remove.hip) places its outputs with too; the wordrow index, the searches
// and the counters in bulk.hpp, the prelude of every bulk mutation.
#include <algorithm>

#include "compact.hpp"

namespace fgpu {

__device__ __forceinline__ bool dt_bit(const u32* __restrict__ bits, u32 v) { return (bits[v >> 5] >> (v & 31)) & 1u; }

// bits[] |= nodes; *n_distinct += the bits that were clear
__global__ __launch_bounds__(256) void dt_bitmap_kernel(const u32* __restrict__ nodes, u64 n, u32* __restrict__ bits,
                                                       u32* __restrict__ n_distinct) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const u32 v = nodes[i], bit = 1u << (v & 31);
        fresh = (atomicOr(&bits[v >> 5], bit) & bit) == 0;
    }
    count_if(fresh, n_distinct);
}

// keep[p] = the entry stays; list[p] (nullable) = the entry goes to this pass's list: its row is in D (row_side) and, with
// excl_col, its column is not.  Position nnz of both is 0, so that the scans end in the totals.
__global__ __launch_bounds__(256) void dt_flag_kernel(CsrView a, const u64* __restrict__ vals, const u32* __restrict__ wordrow, u32 nnz,
                                                     const u32* __restrict__ bits, bool row_side, bool col_side, bool excl_col,
                                                     u32* __restrict__ keep, u32* __restrict__ list, u32* __restrict__ n_multi) {
    const u64 p64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool multi = false;
    if (p64 < nnz) {
        const u32 p = (u32)p64;
        const u32 r = entry_row(a, wordrow, p), c = a.colidx[p];
        const bool dr = row_side && dt_bit(bits, r);
        const bool dc = col_side && dt_bit(bits, c);
        keep[p] = (dr || dc) ? 0u : 1u;
        if (list) list[p] = (dr && !(excl_col && dc)) ? 1u : 0u;
        multi = n_multi && vals && (dr || dc) && vals[p] == ~0ull;
    } else if (p64 == nnz) {
        keep[nnz] = 0u;
        if (list) list[nnz] = 0u;
    }
    if (n_multi) count_if(multi, n_multi);
}

static fgpu_info dt_flags(fgpu_ctx* ctx, DtPass& ps, const fgpu_mat* a, const u32* bits, bool row_side, bool col_side, bool excl_col,
                          bool listed, u32* kept_dev, u32* listed_dev, u32* n_multi_dev) {
    hipStream_t st = ctx->stream();
    ps.a = a;
    ps.listed = listed;
    const u64 nnz = a->nnz;
    FGPU_TRY(ps.E.alloc(ctx, nnz + 1));
    if (listed) FGPU_TRY(ps.O.alloc(ctx, nnz + 1));
    if (nnz == 0) {
        FGPU_HIP(hipMemsetAsync(ps.E.p, 0, sizeof(u32), st));
        if (listed) FGPU_HIP(hipMemsetAsync(ps.O.p, 0, sizeof(u32), st));
        return FGPU_OK;
    }
    ProfScope prof(ctx, "dt_flags", nnz * (a->vals ? 12 : 4) + (listed ? 16 : 8) * nnz);
    FGPU_TRY(ps.index(ctx));
    FGPU_TRY(launch(dt_flag_kernel, dim3(cdiv(nnz + 1, 256)), dim3(256), 0, st, view_of(a), (const u64*)a->vals,
                    (const u32*)ps.wordrow.p, (u32)nnz, bits, row_side, col_side, excl_col, ps.E.p, listed ? ps.O.p : nullptr,
                    n_multi_dev));
    FGPU_TRY(scan_u32(ctx, ps.E.p, ps.E.p, nnz + 1, kept_dev));
    if (listed) FGPU_TRY(scan_u32(ctx, ps.O.p, ps.O.p, nnz + 1, listed_dev));
    return FGPU_OK;
}

static fgpu_info nodes_detach_impl(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const u64* nodes, u64 n_nodes, int sides,
                                   fgpu_mat** m_out, fgpu_mat** mt_out, u64** rem_row, u64** rem_col, u64** rem_val, u64* n_rem,
                                   u64* n_rem_out, u64* stats) {
    FGPU_REQUIRE(ctx && m && m_out, FGPU_NULL_POINTER, "fgpu_nodes_detach: NULL argument");
    *m_out = nullptr;
    if (mt_out) *mt_out = nullptr;
    const bool want_list = rem_row != nullptr;
    if (want_list) {
        FGPU_REQUIRE(rem_col && rem_val && n_rem && n_rem_out, FGPU_NULL_POINTER, "fgpu_nodes_detach: NULL list argument");
        *rem_row = *rem_col = *rem_val = nullptr;
    }
    if (n_rem) *n_rem = 0;
    if (n_rem_out) *n_rem_out = 0;
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(n_nodes == 0 || nodes, FGPU_NULL_POINTER, "fgpu_nodes_detach: NULL node array");
    FGPU_REQUIRE((mt != nullptr) == (mt_out != nullptr), FGPU_NULL_POINTER,
                 "fgpu_nodes_detach: mt_out must be given exactly when mt is");
    FGPU_REQUIRE(sides >= 1 && sides <= 3, FGPU_INVALID, "fgpu_nodes_detach: sides = %d is not 1, 2 or 3", sides);
    FGPU_REQUIRE(!want_list || mt, FGPU_INVALID, "fgpu_nodes_detach: the removal list needs the transposed pattern mt");
    if (mt) FGPU_TRY(require_pattern_of("fgpu_nodes_detach", "mt", mt, m));
    FGPU_REQUIRE(!(want_list && (sides & 2)) || m->nrows == m->ncols, FGPU_INVALID,
                 "fgpu_nodes_detach: a list over both sides needs a square matrix (got %llu x %llu)", (unsigned long long)m->nrows,
                 (unsigned long long)m->ncols);
    FGPU_REQUIRE(n_nodes < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_nodes_detach: %llu nodes exceed the 32-bit id space",
                 (unsigned long long)n_nodes);
    const bool row_side = (sides & 1) != 0, col_side = (sides & 2) != 0;
    std::vector<u32> n32(n_nodes);
    for (u64 i = 0; i < n_nodes; ++i) {
        FGPU_REQUIRE((!row_side || nodes[i] < m->nrows) && (!col_side || nodes[i] < m->ncols), FGPU_INVALID,
                     "fgpu_nodes_detach: node %llu (position %llu) is outside the %llu x %llu matrix", (unsigned long long)nodes[i],
                     (unsigned long long)i, (unsigned long long)m->nrows, (unsigned long long)m->ncols);
        n32[i] = (u32)nodes[i];
    }
    hipStream_t st = ctx->stream();
    // ---- bitmap ---------------------------------------------------------------------------------------------------------
    const u64 nbits = std::max(m->nrows, m->ncols);
    const size_t bwords = (size_t)((nbits + 31) >> 5) + 1;
    DevBuf<u32> bits, tot, dnodes;
    FGPU_TRY(bits.alloc(ctx, bwords));
    FGPU_TRY(tot.alloc(ctx, 8));   // [0] kept in m [1] out entries [2] kept in mt [3] in entries [4] distinct nodes [5] MULTI_EDGE removed
    FGPU_HIP(hipMemsetAsync(bits.p, 0, bwords * sizeof(u32), st));
    FGPU_HIP(hipMemsetAsync(tot.p, 0, 8 * sizeof(u32), st));
    if (n_nodes) {
        FGPU_TRY(dnodes.alloc(ctx, n_nodes));
        FGPU_TRY(ctx->h2d(dnodes.p, n32.data(), n_nodes * sizeof(u32)));
        FGPU_TRY(launch(dt_bitmap_kernel, dim3(cdiv(n_nodes, 256)), dim3(256), 0, st, (const u32*)dnodes.p, n_nodes, bits.p, tot.p + 4));
    }
    // ---- flags and scans ------------------------------------------------------------------------------------------------
    DtPass pm, pt;
    FGPU_TRY(dt_flags(ctx, pm, m, bits.p, row_side, col_side, false, want_list, tot.p + 0, tot.p + 1, tot.p + 5));
    // (the transposed pattern: its rows are m's columns, so the sides swap; an entry whose column — m's row — is in D too is
    // an out entry and stays out of the in-list)
    if (mt) FGPU_TRY(dt_flags(ctx, pt, mt, bits.p, col_side, row_side, true, want_list, tot.p + 2, tot.p + 3, nullptr));
    u32 h[6];
    FGPU_TRY(read_words(ctx, tot.p, 6, h));
    if (m->nnz == 0) h[0] = h[1] = 0;
    if (!mt || mt->nnz == 0) h[2] = h[3] = 0;
    const u64 kept_m = h[0], n_out = want_list ? h[1] : 0, kept_t = h[2], n_in = want_list ? h[3] : 0, n_list = n_out + n_in;
    // ---- outputs --------------------------------------------------------------------------------------------------------
    DevBuf<u32> lrow, lcol;
    DevBuf<u64> lval;
    if (n_list) {
        FGPU_TRY(lrow.alloc(ctx, n_list));
        FGPU_TRY(lcol.alloc(ctx, n_list));
        FGPU_TRY(lval.alloc(ctx, n_list));
    }
    MatRef om, ot;
    FGPU_TRY(dt_emit(ctx, pm, kept_m, om, lrow.p, lcol.p, lval.p, 0, false, nullptr));
    if (mt) FGPU_TRY(dt_emit(ctx, pt, kept_t, ot, lrow.p, lcol.p, lval.p, (u32)n_out, true, m));
    ResultBuf rr, rc, rv;
    if (n_list) {
        ProfScope prof(ctx, "dt_readback", 16 * n_list);
        FGPU_REQUIRE(rr.alloc(ctx, n_list * sizeof(u64)) && rc.alloc(ctx, n_list * sizeof(u64)) && rv.alloc(ctx, n_list * sizeof(u64)),
                     FGPU_OOM, "fgpu_nodes_detach: out of host memory");
        FGPU_TRY(ctx->d2h_widen((u64*)rr.p, lrow.p, n_list));
        FGPU_TRY(ctx->d2h_widen((u64*)rc.p, lcol.p, n_list));
        FGPU_TRY(ctx->d2h((u64*)rv.p, lval.p, n_list * sizeof(u64)));
    }
    if (stats) {
        stats[0] = h[4];
        stats[1] = n_out;
        stats[2] = n_in;
        stats[3] = h[5];
        stats[4] = kept_m;
        stats[5] = kept_t;
    }
    *m_out = om.release();
    if (mt) *mt_out = ot.release();
    if (want_list) {
        *rem_row = (u64*)rr.release();
        *rem_col = (u64*)rc.release();
        *rem_val = (u64*)rv.release();
        *n_rem = n_list;
        *n_rem_out = n_out;
    }
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_nodes_detach(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* nodes, uint64_t n_nodes,
                                       int sides, fgpu_mat** m_out, fgpu_mat** mt_out, uint64_t** rem_row, uint64_t** rem_col,
                                       uint64_t** rem_val, uint64_t* n_rem, uint64_t* n_rem_out, uint64_t stats[8]) {
    return published(ctx, nodes_detach_impl(ctx, m, mt, nodes, n_nodes, sides, m_out, mt_out, rem_row, rem_col, rem_val, n_rem,
                                            n_rem_out, stats));
}
