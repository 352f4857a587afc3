// compact.hpp — the compaction half shared by detach.hip (fgpu_nodes_detach) and edges_remove.hip (fgpu_edges_remove): both
// decide keep or drop per stored entry position of a snapshot, scan the flags, and place everything by the scan.
//
//   wordrow  the per-call index of bulk.hpp over the pass's matrix (dt_wordrow)
//   E        the exclusive scan of keep over nnz + 1 flags (keep[nnz] = 0), so that E[nnz] is the number of kept entries;
//            entry p stays exactly when E[p + 1] != E[p], and then goes to position E[p] of the output
//   rows     rowptr'[r] = E[rowptr[r]], a lane per row — no per-row loop; a hypersparse input goes through its hrows, and the
//            output is hypersparse exactly when fgpu_mat_from_coo would store that many populated rows so (mat_prefer_hyper)
//
// The kernels are static: each translation unit carries its own copy.  The searches, the counters and the marshalling of the
// callers' arrays are bulk.hpp's, which this file includes; edges_union.hip (fgpu_edges_union) and edges.hip (fgpu_edges_build)
// compact nothing and include bulk.hpp alone.
#pragma once
#include "bulk.hpp"

namespace fgpu {

// E / O: the scans of keep / list.  A kept entry goes to out_col / out_val; a listed one to lrow / lcol / lval at lbase + O[p] —
// as (row, col, value) of this matrix, or with `swap` (the pass over the transposed pattern) as (col, row, value of (col, row) in
// the forward matrix fwd)
static __global__ __launch_bounds__(256) void dt_emit_kernel(CsrView a, const u64* __restrict__ vals, const u32* __restrict__ wordrow,
                                                            u32 nnz, const u32* __restrict__ E, const u32* __restrict__ O,
                                                            u32* __restrict__ out_col, u64* __restrict__ out_val,
                                                            u32* __restrict__ lrow, u32* __restrict__ lcol, u64* __restrict__ lval,
                                                            u32 lbase, bool swap, CsrView fwd, const u64* __restrict__ fwd_vals) {
    const u64 p64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p64 >= nnz) return;
    const u32 p = (u32)p64;
    const u32 c = a.colidx[p];
    const u32 e0 = E[p];
    if (E[p + 1] != e0) {
        out_col[e0] = c;
        if (out_val) out_val[e0] = vals[p];
    }
    if (!O) return;
    const u32 o0 = O[p];
    if (O[p + 1] == o0) return;
    const u32 r = entry_row(a, wordrow, p);
    const u32 at = lbase + o0;
    if (!swap) {
        lrow[at] = r;
        lcol[at] = c;
        lval[at] = vals ? vals[p] : 0ull;
        return;
    }
    u64 v = 0;
    if (fwd_vals) {
        const u32 q = probe(fwd, c, r);
        if (q != ~0u) v = fwd_vals[q];
    }
    lrow[at] = c;
    lcol[at] = r;
    lval[at] = v;
}

// F[i] = stored row i keeps an entry (i < nvec); F[nvec] = 0
static __global__ __launch_bounds__(256) void dt_rowflag_kernel(const u32* __restrict__ rp, u32 nvec, const u32* __restrict__ E,
                                                               u32* __restrict__ F) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i > nvec) return;
    F[i] = (i < nvec && E[rp[i + 1]] != E[rp[i]]) ? 1u : 0u;
}

// the hypersparse output: stored row i of the input that keeps an entry becomes stored row F[i] (F scanned)
static __global__ __launch_bounds__(256) void dt_rows_hyper_kernel(const u32* __restrict__ rp, const u32* __restrict__ hrows, u32 nvec,
                                                                  const u32* __restrict__ E, const u32* __restrict__ F, u32 nvec_out,
                                                                  u32 kept, u32* __restrict__ rp_out, u32* __restrict__ hr_out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i > nvec) return;
    if (i == nvec) { rp_out[nvec_out] = kept; return; }
    const u32 e0 = E[rp[i]];
    if (E[rp[i + 1]] == e0) return;
    const u32 at = F[i];
    rp_out[at] = e0;
    hr_out[at] = hrows ? hrows[i] : i;
}

// the full output: rowptr'[r] = E[first entry of the first stored row at or past r]
static __global__ __launch_bounds__(256) void dt_rows_full_kernel(const u32* __restrict__ rp, const u32* __restrict__ hrows, u32 nvec,
                                                                 u64 nrows, const u32* __restrict__ E, u32* __restrict__ rp_out) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    rp_out[r] = E[rp[hrows ? lower_bound(hrows, 0u, nvec, (u32)r) : (u32)r]];
}

// one matrix' pass, in two halves around the read-back of the totals: its flags and scans are the caller's, dt_emit is shared
struct DtPass {
    const fgpu_mat* a = nullptr;
    DevBuf<u32> wordrow, E, O;
    bool listed = false;
    // wordrow of a (which holds an entry)
    fgpu_info index(fgpu_ctx* ctx) { return wordrow_build(ctx, a->rowptr, a->nvec, a->nnz, wordrow); }
};

// the output snapshot of a pass (its row pointers here, its entries by dt_emit_kernel), then the emission
static fgpu_info dt_emit(fgpu_ctx* ctx, DtPass& ps, u64 kept, MatRef& out, u32* lrow, u32* lcol, u64* lval, u32 lbase, bool swap,
                         const fgpu_mat* fwd) {
    hipStream_t st = ctx->stream();
    const fgpu_mat* a = ps.a;
    const u32 nvec = a->nvec;
    const u64 nrows = a->nrows;
    u32 nvec_out = 0;
    bool hyper = false;
    DevBuf<u32> F;
    if (nrows > HYPER_MIN_ROWS) {
        FGPU_TRY(F.alloc(ctx, (size_t)nvec + 1));
        DevBuf<u32> tot;
        FGPU_TRY(tot.alloc(ctx, 1));
        FGPU_TRY(launch(dt_rowflag_kernel, dim3(cdiv((u64)nvec + 1, 256)), dim3(256), 0, st, (const u32*)a->rowptr, nvec,
                        (const u32*)ps.E.p, F.p));
        FGPU_TRY(scan_u32(ctx, F.p, F.p, (u64)nvec + 1, tot.p));
        FGPU_TRY(read_u32(ctx, tot.p, &nvec_out));
        hyper = mat_prefer_hyper(nrows, nvec_out);
    }
    FGPU_TRY(mat_alloc(ctx, &out.m, nrows, a->ncols, kept, a->vals != nullptr, nvec_out, hyper));
    if (hyper) {
        FGPU_TRY(launch(dt_rows_hyper_kernel, dim3(cdiv((u64)nvec + 1, 256)), dim3(256), 0, st, (const u32*)a->rowptr,
                        (const u32*)a->hrows, nvec, (const u32*)ps.E.p, (const u32*)F.p, nvec_out, (u32)kept, out->rowptr, out->hrows));
    } else {
        FGPU_TRY(launch(dt_rows_full_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, st, (const u32*)a->rowptr, (const u32*)a->hrows,
                        nvec, nrows, (const u32*)ps.E.p, out->rowptr));
    }
    if (a->nnz == 0) return FGPU_OK;
    ProfScope prof(ctx, "dt_emit", a->nnz * (a->vals ? 20 : 12) + kept * (a->vals ? 12 : 4));
    CsrView fv = fwd ? view_of(fwd) : view_of(a);
    FGPU_TRY(launch(dt_emit_kernel, dim3(cdiv(a->nnz, 256)), dim3(256), 0, st, view_of(a), (const u64*)a->vals, (const u32*)ps.wordrow.p,
                    (u32)a->nnz, (const u32*)ps.E.p, ps.listed ? (const u32*)ps.O.p : nullptr, out->colidx, out->vals, lrow, lcol, lval,
                    lbase, swap, fv, fwd ? (const u64*)fwd->vals : nullptr));
    return FGPU_OK;
}

}  // namespace fgpu
