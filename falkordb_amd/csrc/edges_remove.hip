// edges_remove.hip — fgpu_edges_remove: a batch of (src, dst, edge id) triples leaves one relationship type's tensor (DELETE r).
// The reference does this edge list by edge list: Graph::delete_relationships (graph.rs:2268-2373) groups the ids by type and
// hands each group to Tensor::remove_all (tensor.rs:454-629), whose slow path replays every touched pair's transitions — inline
// id removed, multi-edge row shrunk, demoted back to an inline id, emptied.  That path applies a removal only where the id is
// actually there, so it is a set operation and the order of the batch does not matter.  Here one call gives the compacted
// matrix, the compacted transposed pattern, the hit flags and the emptied pairs:
//
//   triples  a lane per triple: binary search of row src of m for dst (hypersparse rows through hrows).  An inline value equal
//            to the id stores keep[p] = 0 and, after the same search of row dst of mt, keep_t[q] = 0; FGPU_MULTI_EDGE searches
//            the supplied keys, then the pair's run for the id, and stores taken[j] = 1.  The flags are u32, keep / keep_t
//            prefilled with 1 and taken with 0: several lanes storing the same value is the only race
//   runs     S = exclusive scan of taken; a lane per supplied multi-edge row: removed = S[off[r + 1]] - S[off[r]].  Nothing left:
//            the pair's keep and keep_t flags go to 0 (two searches).  One left: the survivor is found by a binary search on
//            the monotone count of untaken ids before j — no loop over a hub pair's run — and recorded beside its position p
//   place    E = exclusive scan of keep, the emission, the row pointers and the hypersparse decision are fgpu_nodes_detach's
//            (compact.hpp); then a lane per supplied row patches out_val[E[p]] of the demoted pairs
//   emptied  the compaction of !keep over m: entry p goes to position p - E[p], ascending in (src, dst) without a sort
//
// The only atomics are counters that place nothing (a ballot and one atomicAdd per wavefront).  No wavefront per row or per run.
#include "compact.hpp"

namespace fgpu {

// keep[p] = 1 for p < nnz, keep[nnz] = 0 (so that the scan ends in the total)
__global__ __launch_bounds__(256) void er_fill_kernel(u32* __restrict__ keep, u32 nnz) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p <= nnz) keep[p] = p < nnz ? 1u : 0u;
}

// cnt: [0] hits [1] pair absent [2] pair stored, id unknown [3] MULTI_EDGE pair without a supplied row
__global__ __launch_bounds__(256) void er_triple_kernel(CsrView m, const u64* __restrict__ vals, CsrView mt,
                                                       const u32* __restrict__ srcs, const u32* __restrict__ dsts,
                                                       const u64* __restrict__ ids, u32 n, const u64* __restrict__ mkey,
                                                       const u32* __restrict__ moff, const u64* __restrict__ mids, u32 n_multi,
                                                       u32* __restrict__ keep, u32* __restrict__ keep_t, u32* __restrict__ taken,
                                                       uint8_t* __restrict__ hit, u32* __restrict__ cnt) {
    const u64 k64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool is_hit = false, absent = false, unknown = false, missing = false;
    if (k64 < n) {
        const u32 k = (u32)k64, s = srcs[k], d = dsts[k];
        const u64 id = ids[k];
        const u32 p = probe(m, s, d);
        if (p == ~0u) {
            absent = true;
        } else {
            const u64 v = vals[p];
            if (v != FGPU_MULTI_EDGE) {
                if (v == id) {
                    is_hit = true;
                    keep[p] = 0u;
                    const u32 q = probe(mt, d, s);
                    if (q != ~0u) keep_t[q] = 0u;
                } else {
                    unknown = true;
                }
            } else {
                const u32 r = find(mkey, 0u, n_multi, ((u64)s << 32) | d);
                if (r == ~0u) {
                    missing = true;
                } else {
                    const u32 j = find(mids, moff[r], moff[r + 1], id);
                    if (j != ~0u) { is_hit = true; taken[j] = 1u; }
                    else unknown = true;
                }
            }
        }
        if (hit) hit[k] = is_hit ? 1 : 0;
    }
    count_if(is_hit, cnt + 0);
    count_if(absent, cnt + 1);
    count_if(unknown, cnt + 2);
    count_if(missing, cnt + 3);
}

// a lane per supplied row; S = the scan of taken.  dem_p (prefilled ~0u) / dem_id: position in m and surviving id of a demoted
// pair.  cnt: [0] multi-edge pairs emptied [1] pairs demoted
__global__ __launch_bounds__(256) void er_multi_kernel(CsrView m, const u64* __restrict__ vals, CsrView mt,
                                                      const u64* __restrict__ mkey, const u32* __restrict__ moff,
                                                      const u64* __restrict__ mids, u32 n_multi, const u32* __restrict__ S,
                                                      u32* __restrict__ keep, u32* __restrict__ keep_t, u32* __restrict__ dem_p,
                                                      u64* __restrict__ dem_id, u32* __restrict__ cnt) {
    const u64 r64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool emptied = false, demoted = false;
    if (r64 < n_multi) {
        const u32 r = (u32)r64, b = moff[r], e = moff[r + 1];
        const u32 sb = S[b], removed = S[e] - sb;
        if (removed) {   // (some triple hit an id of the row, so the pair is a MULTI_EDGE entry of m)
            const u64 key = mkey[r];
            const u32 s = (u32)(key >> 32), d = (u32)key;
            const u32 p = probe(m, s, d);
            const u32 left = e - b - removed;
            if (p != ~0u && vals[p] == FGPU_MULTI_EDGE && left <= 1) {
                if (left == 0) {
                    emptied = true;
                    keep[p] = 0u;
                    const u32 q = probe(mt, d, s);
                    if (q != ~0u) keep_t[q] = 0u;
                } else {
                    // untaken ids in [b, j] = (j + 1 - b) - (S[j + 1] - S[b]), ascending in j: the survivor is the first j at 1
                    u32 lo = b, hi = e - 1;
                    while (lo < hi) {
                        const u32 mid = lo + ((hi - lo) >> 1);
                        if ((mid + 1 - b) - (S[mid + 1] - sb) >= 1u) hi = mid; else lo = mid + 1;
                    }
                    demoted = true;
                    dem_p[r] = p;
                    dem_id[r] = mids[lo];
                }
            }
        }
    }
    count_if(emptied, cnt + 0);
    count_if(demoted, cnt + 1);
}

// multi_taken[j] = taken[j], read off its scan
__global__ __launch_bounds__(256) void er_taken_kernel(const u32* __restrict__ S, u32 total, uint8_t* __restrict__ out) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j < total) out[j] = (uint8_t)(S[j + 1] - S[j]);
}

// the demoted pairs of the output: the surviving id inline
__global__ __launch_bounds__(256) void er_patch_kernel(const u32* __restrict__ dem_p, const u64* __restrict__ dem_id, u32 n_multi,
                                                      const u32* __restrict__ E, u64* __restrict__ out_val) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_multi) return;
    const u32 p = dem_p[r];
    if (p != ~0u) out_val[E[p]] = dem_id[r];
}

// the dropped entries of m as (row, col), entry p at position p - E[p]
__global__ __launch_bounds__(256) void er_emptied_kernel(CsrView a, const u32* __restrict__ wordrow, u32 nnz, const u32* __restrict__ E,
                                                        u32* __restrict__ lrow, u32* __restrict__ lcol) {
    const u64 p64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p64 >= nnz) return;
    const u32 p = (u32)p64, e0 = E[p];
    if (E[p + 1] != e0) return;
    lrow[p - e0] = entry_row(a, wordrow, p);
    lcol[p - e0] = a.colidx[p];
}

static fgpu_info er_fill(fgpu_ctx* ctx, DtPass& ps, const fgpu_mat* a) {
    ps.a = a;
    FGPU_TRY(ps.E.alloc(ctx, a->nnz + 1));
    return launch(er_fill_kernel, dim3(cdiv(a->nnz + 1, 256)), dim3(256), 0, ctx->stream(), ps.E.p, (u32)a->nnz);
}

static fgpu_info edges_remove_impl(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const u64* srcs, const u64* dsts,
                                   const u64* ids, u64 n, const u64* multi_key, const u64* multi_off, const u64* multi_ids,
                                   u64 n_multi, fgpu_mat** m_out, fgpu_mat** mt_out, uint8_t* hit, uint8_t* multi_taken,
                                   u64** emp_row, u64** emp_col, u64* n_emp, u64* stats) {
    FGPU_REQUIRE(ctx && m && m_out && mt_out && emp_row && emp_col && n_emp, FGPU_NULL_POINTER, "fgpu_edges_remove: NULL argument");
    *m_out = *mt_out = nullptr;
    *emp_row = *emp_col = nullptr;
    *n_emp = 0;
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(n == 0 || (srcs && dsts && ids), FGPU_NULL_POINTER, "fgpu_edges_remove: NULL triple arrays");
    FGPU_REQUIRE(n_multi == 0 || (multi_key && multi_off && multi_ids && multi_taken), FGPU_NULL_POINTER,
                 "fgpu_edges_remove: NULL multi-edge rows or multi_taken");
    FGPU_REQUIRE(m->vals, FGPU_INVALID, "fgpu_edges_remove: m must be the tensor's UINT64 base (got a BOOL matrix)");
    FGPU_TRY(require_pattern_of("fgpu_edges_remove", "mt", mt, m));
    FGPU_REQUIRE(n < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_edges_remove: %llu triples exceed the 32-bit position space",
                 (unsigned long long)n);
    FGPU_REQUIRE(n_multi < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_edges_remove: %llu multi-edge rows exceed the 32-bit position space",
                 (unsigned long long)n_multi);
    std::vector<u32> s32, d32;
    FGPU_TRY(marshal_triples("fgpu_edges_remove", srcs, dsts, ids, n, m->nrows, m->ncols, s32, d32));
    MultiRows rows;
    FGPU_TRY(rows.check("fgpu_edges_remove", "multi", multi_key, multi_off, multi_ids, n_multi));
    const u64 T = rows.total();
    hipStream_t st = ctx->stream();
    // ---- flags ----------------------------------------------------------------------------------------------------------
    DevBuf<u32> tot, dsrc, ddst, taken, dem_p;
    DevBuf<u64> dids, dem_id;
    DevBuf<uint8_t> dhit, dtaken8;
    // [0] kept in m [1] kept in mt [2] hits [3] absent [4] unknown [5] MULTI_EDGE without a row [6] multi emptied [7] demoted
    FGPU_TRY(tot.alloc(ctx, 8));
    FGPU_HIP(hipMemsetAsync(tot.p, 0, 8 * sizeof(u32), st));
    DtPass pm, pt;
    FGPU_TRY(er_fill(ctx, pm, m));
    FGPU_TRY(er_fill(ctx, pt, mt));
    if (n_multi) {
        FGPU_TRY(taken.alloc(ctx, T + 1));
        FGPU_TRY(dem_p.alloc(ctx, n_multi));
        FGPU_TRY(dem_id.alloc(ctx, n_multi));
        FGPU_TRY(rows.upload(ctx, "er_h2d"));
        FGPU_HIP(hipMemsetAsync(taken.p, 0, (T + 1) * sizeof(u32), st));
        FGPU_HIP(hipMemsetAsync(dem_p.p, 0xFF, n_multi * sizeof(u32), st));
    }
    if (n) {
        FGPU_TRY(dsrc.alloc(ctx, n));
        FGPU_TRY(ddst.alloc(ctx, n));
        FGPU_TRY(dids.alloc(ctx, n));
        if (hit) FGPU_TRY(dhit.alloc(ctx, n));
        {
            ProfScope up(ctx, "er_h2d", n * 16);
            FGPU_TRY(ctx->h2d(dsrc.p, s32.data(), n * sizeof(u32)));
            FGPU_TRY(ctx->h2d(ddst.p, d32.data(), n * sizeof(u32)));
            FGPU_TRY(ctx->h2d(dids.p, ids, n * sizeof(u64)));
        }
        ProfScope prof(ctx, "er_triples", n * 16);   // (plus one 64-byte line per probe step: the searches are the cost)
        FGPU_TRY(launch(er_triple_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, view_of(m), (const u64*)m->vals, view_of(mt),
                        (const u32*)dsrc.p, (const u32*)ddst.p, (const u64*)dids.p, (u32)n, (const u64*)rows.key.p, (const u32*)rows.off.p,
                        (const u64*)rows.ids.p, (u32)n_multi, pm.E.p, pt.E.p, taken.p, dhit.p, tot.p + 2));
    }
    if (n_multi) {
        ProfScope prof(ctx, "er_multi", T * 8 + n_multi * 24);
        FGPU_TRY(scan_u32(ctx, taken.p, taken.p, T + 1, nullptr));
        FGPU_TRY(launch(er_multi_kernel, dim3(cdiv(n_multi, 256)), dim3(256), 0, st, view_of(m), (const u64*)m->vals, view_of(mt),
                        (const u64*)rows.key.p, (const u32*)rows.off.p, (const u64*)rows.ids.p, (u32)n_multi, (const u32*)taken.p, pm.E.p,
                        pt.E.p, dem_p.p, dem_id.p, tot.p + 6));
    }
    {
        ProfScope prof(ctx, "er_scans", 8 * (m->nnz + mt->nnz));
        FGPU_TRY(scan_u32(ctx, pm.E.p, pm.E.p, m->nnz + 1, tot.p + 0));
        FGPU_TRY(scan_u32(ctx, pt.E.p, pt.E.p, mt->nnz + 1, tot.p + 1));
    }
    u32 h[8];
    FGPU_TRY(read_words(ctx, tot.p, 8, h));
    FGPU_REQUIRE(h[5] == 0, FGPU_INVALID,
                 "fgpu_edges_remove: %u triples name a pair that holds MULTI_EDGE in m, and no multi-edge row was supplied for it", h[5]);
    const u64 kept_m = h[0], kept_t = h[1], emptied = m->nnz - kept_m;
    // ---- outputs --------------------------------------------------------------------------------------------------------
    DevBuf<u32> lrow, lcol;
    ResultBuf rr, rc;
    if (emptied) {
        FGPU_TRY(lrow.alloc(ctx, emptied));
        FGPU_TRY(lcol.alloc(ctx, emptied));
        FGPU_REQUIRE(rr.alloc(ctx, emptied * sizeof(u64)) && rc.alloc(ctx, emptied * sizeof(u64)), FGPU_OOM,
                     "fgpu_edges_remove: out of host memory");
        FGPU_TRY(pm.index(ctx));
    }
    if (n_multi) FGPU_TRY(dtaken8.alloc(ctx, T));
    MatRef om, ot;
    FGPU_TRY(dt_emit(ctx, pm, kept_m, om, nullptr, nullptr, nullptr, 0, false, nullptr));
    FGPU_TRY(dt_emit(ctx, pt, kept_t, ot, nullptr, nullptr, nullptr, 0, false, nullptr));
    if (h[7])
        FGPU_TRY(launch(er_patch_kernel, dim3(cdiv(n_multi, 256)), dim3(256), 0, st, (const u32*)dem_p.p, (const u64*)dem_id.p,
                        (u32)n_multi, (const u32*)pm.E.p, om->vals));
    if (emptied) {
        ProfScope prof(ctx, "er_emptied", m->nnz * 8 + emptied * 8);
        FGPU_TRY(launch(er_emptied_kernel, dim3(cdiv(m->nnz, 256)), dim3(256), 0, st, view_of(m), (const u32*)pm.wordrow.p, (u32)m->nnz,
                        (const u32*)pm.E.p, lrow.p, lcol.p));
    }
    if (n_multi) FGPU_TRY(launch(er_taken_kernel, dim3(cdiv(T, 256)), dim3(256), 0, st, (const u32*)taken.p, (u32)T, dtaken8.p));
    {
        ProfScope prof(ctx, "er_readback", emptied * 16 + T + (hit ? n : 0));
        if (emptied) {
            FGPU_TRY(ctx->d2h_widen((u64*)rr.p, lrow.p, emptied));
            FGPU_TRY(ctx->d2h_widen((u64*)rc.p, lcol.p, emptied));
        }
        if (n_multi) FGPU_TRY(ctx->d2h(multi_taken, dtaken8.p, T));
        if (hit && n) FGPU_TRY(ctx->d2h(hit, dhit.p, n));
    }
    if (stats) {
        stats[0] = h[2];
        stats[1] = emptied;
        stats[2] = h[6];
        stats[3] = h[7];
        stats[4] = kept_m;
        stats[5] = kept_t;
        stats[6] = h[3];
        stats[7] = h[4];
    }
    *m_out = om.release();
    *mt_out = ot.release();
    *emp_row = (u64*)rr.release();
    *emp_col = (u64*)rc.release();
    *n_emp = emptied;
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_edges_remove(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* srcs, const uint64_t* dsts,
                                       const uint64_t* ids, uint64_t n, const uint64_t* multi_key, const uint64_t* multi_off,
                                       const uint64_t* multi_ids, uint64_t n_multi, fgpu_mat** m_out, fgpu_mat** mt_out, uint8_t* hit,
                                       uint8_t* multi_taken, uint64_t** emp_row, uint64_t** emp_col, uint64_t* n_emp,
                                       uint64_t stats[8]) {
    return published(ctx, edges_remove_impl(ctx, m, mt, srcs, dsts, ids, n, multi_key, multi_off, multi_ids, n_multi, m_out, mt_out,
                                            hit, multi_taken, emp_row, emp_col, n_emp, stats));
}
