// edges_union.hip — fgpu_edges_union: one built batch (fgpu_edges_build's fwd / bwd / rows) joins a tensor that already holds
// edges (CREATE onto a loaded graph).  The reference does this edge by edge in Tensor::set_all_from_slices (tensor.rs:333-447,
// under Graph::create_relationships_bulk, graph.rs:2062-2121): per edge it reads the pair's state — absent, an inline id, or
// MULTI_EDGE — and either stores the id inline, promotes the pair (both ids go to the me row, the entry becomes MULTI_EDGE) or
// extends the row (tensor.rs:383-418).  On sets that is a union per pair: a pair only the batch names enters with the batch's
// value; a pair stored on both sides ends MULTI_EDGE with the ascending merge of both id lists; the rest of m stays.
//
//   classify  a lane per stored entry q of fwd (its row from the wordrow index of bulk.hpp, hrows included): binary search of
//             row src of m for dst gives lb[q], the entry of m it meets or the position it would be inserted at.  Met = the pair
//             collides: each side is its inline id or, under MULTI_EDGE, the supplied row found by a search of a_key / b_key.
//             The same search of bwd's entries in mt, without the sides
//   scans     N = scan(new), C = scan(collide), L = scan(collide ? lenA + lenB : 0): the place of every new entry, the out row
//             of every colliding pair and its offset.  Totals and the missing-row counters come back in one read
//   ids       a lane per OUTPUT id: its row between idrow[t / 64] and idrow[t / 64 + 1] (the row of every 64th id), its element
//             by a co-rank (merge path) binary search over the two sorted sides — a pair of 10^5 ids is 10^5 lanes of 17 steps.
//             Equal ids at the split are an id stored on both sides: counted, read back before any output is allocated
//   place     m_out = m U fwd: entry p of m goes to p + (new entries inserted at or before p) — a histogram of lb over the new
//             entries, scanned — and entry q of fwd to lb[q] + N[q], written after m's so that the batch's entry wins
//             (MULTI_EDGE at a colliding pair).  rowptr'[r] = rowptr_m[r] + N[rowptr_fwd[r]], a lane per row; the populated rows
//             are one more flag and scan, and the output is hypersparse exactly when fgpu_mat_from_coo would store it so.
//             mt_out = mt U bwd is the same placement without values
//
// A lane per item everywhere, no wavefront or loop per row or per run.  The atomics count: a ballot and one add per wavefront
// for the counters, one add per new entry into the histogram that the scan turns into shifts.  They place nothing.
#include "bulk.hpp"

namespace fgpu {

// a lane per entry q of fwd (q == nnz: the closing zeros of the three scans).
// cnt: [0] promoted [1] extended [2] MULTI_EDGE in m without an a row [3] MULTI_EDGE in fwd without a b row
__global__ __launch_bounds__(256) void eu_classify_kernel(CsrView m, const u64* __restrict__ mvals, CsrView f,
                                                         const u64* __restrict__ fvals, const u32* __restrict__ wordrow, u32 nnz,
                                                         const u64* __restrict__ akey, const u32* __restrict__ aoff, u32 n_a,
                                                         const u64* __restrict__ bkey, const u32* __restrict__ boff, u32 n_b,
                                                         u32* __restrict__ lb, u32* __restrict__ isnew, u32* __restrict__ collide,
                                                         u32* __restrict__ len, u32* __restrict__ startA, u32* __restrict__ lenA,
                                                         u32* __restrict__ startB, u32* __restrict__ cnt) {
    const u64 q64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool promoted = false, extended = false, missA = false, missB = false;
    if (q64 == nnz) isnew[nnz] = collide[nnz] = len[nnz] = 0u;
    if (q64 < nnz) {
        const u32 q = (u32)q64;
        const u32 src = entry_row(f, wordrow, q), dst = f.colidx[q];
        bool found;
        const u32 p = locate(m, src, dst, found);
        u32 la = 0, sa = 0, lbn = 0, sb = 0;
        if (found) {
            const u64 key = ((u64)src << 32) | dst;
            if (mvals[p] != FGPU_MULTI_EDGE) {
                promoted = true;
                la = 1u;
                sa = p;
            } else {
                extended = true;
                const u32 r = find(akey, 0u, n_a, key);
                if (r == ~0u) missA = true;
                else { sa = aoff[r]; la = aoff[r + 1] - sa; }
            }
            if (fvals[q] != FGPU_MULTI_EDGE) {
                lbn = 1u;
                sb = q;
            } else {
                const u32 r = find(bkey, 0u, n_b, key);
                if (r == ~0u) missB = true;
                else { sb = boff[r]; lbn = boff[r + 1] - sb; }
            }
        }
        lb[q] = p;
        isnew[q] = found ? 0u : 1u;
        collide[q] = found ? 1u : 0u;
        len[q] = la + lbn;
        startA[q] = sa;
        lenA[q] = la;
        startB[q] = sb;
    }
    count_if(promoted, cnt + 0);
    count_if(extended, cnt + 1);
    count_if(missA, cnt + 2);
    count_if(missB, cnt + 3);
}

// the pattern side: a lane per entry q of bwd against mt
__global__ __launch_bounds__(256) void eu_locate_kernel(CsrView a, CsrView b, const u32* __restrict__ wordrow, u32 nnz,
                                                       u32* __restrict__ lb, u32* __restrict__ isnew) {
    const u64 q64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q64 > nnz) return;
    if (q64 == nnz) { isnew[nnz] = 0u; return; }
    const u32 q = (u32)q64;
    bool found;
    lb[q] = locate(a, entry_row(b, wordrow, q), b.colidx[q], found);
    isnew[q] = found ? 0u : 1u;
}

// a lane per entry q of fwd; C / L: the scans of collide / len.  A colliding pair fills its out row C[q]
__global__ __launch_bounds__(256) void eu_rows_kernel(CsrView f, const u32* __restrict__ wordrow, u32 nnz, const u32* __restrict__ C,
                                                     const u32* __restrict__ L, u32 n_o, u32* __restrict__ rowq,
                                                     u64* __restrict__ okey, u32* __restrict__ ooff, u32* __restrict__ longest) {
    const u64 q64 = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 mine = 0;
    if (q64 < nnz) {
        const u32 q = (u32)q64;
        if (q == 0) ooff[n_o] = L[nnz];
        const u32 r = C[q];
        if (C[q + 1] != r) {
            rowq[r] = q;
            okey[r] = ((u64)entry_row(f, wordrow, q) << 32) | f.colidx[q];
            ooff[r] = L[q];
            mine = L[q + 1] - L[q];
        }
    }
    for (u32 d = 32; d >= 1; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)mine, (int)d);
        mine = o > mine ? o : mine;
    }
    if (lane_id() == 0 && mine) atomicMax(longest, mine);
}

// a lane per output id t: row r by the idrow index, element t - ooff[r] of the merge of the row's two sides by co-rank
__global__ __launch_bounds__(256) void eu_ids_kernel(const u32* __restrict__ ooff, const u32* __restrict__ idrow, u32 total,
                                                    const u32* __restrict__ rowq, const u32* __restrict__ startA,
                                                    const u32* __restrict__ lenA, const u32* __restrict__ startB,
                                                    const u64* __restrict__ mvals, const u64* __restrict__ aids,
                                                    const u64* __restrict__ fvals, const u64* __restrict__ bids,
                                                    u64* __restrict__ out, u32* __restrict__ both) {
    const u64 t64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool equal = false;
    if (t64 < total) {
        const u32 t = (u32)t64, r = entry_vec(ooff, idrow, t);
        const u32 o0 = ooff[r], k = t - o0, q = rowq[r];
        const u32 la = lenA[q], lbn = ooff[r + 1] - o0 - la;
        const u64* __restrict__ A = (la == 1u ? mvals : aids) + startA[q];    // (a supplied row holds at least 2 ids)
        const u64* __restrict__ B = (lbn == 1u ? fvals : bids) + startB[q];
        // i = ids of A among the first k of the merge (A first on a tie): the least i with A[i] > B[k - i - 1]
        u32 lo = k > lbn ? k - lbn : 0u, hi = k < la ? k : la;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (A[mid] <= B[k - mid - 1]) lo = mid + 1; else hi = mid;
        }
        const u32 i = lo, j = k - lo;
        const u64 x = i < la ? A[i] : ~0ull, y = j < lbn ? B[j] : ~0ull;
        equal = i < la && j < lbn && x == y;
        out[t] = (j >= lbn || (i < la && x <= y)) ? x : y;
    }
    count_if(equal, both);
}

// H[lb[q]] += 1 for every new entry q of the batch: the scan of H is the shift of the base's entries
__global__ __launch_bounds__(256) void eu_hist_kernel(const u32* __restrict__ lb, const u32* __restrict__ N, u32 nnz,
                                                     u32* __restrict__ H) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q < nnz && N[q + 1] != N[q]) atomicAdd(H + lb[q], 1u);
}

// X: the exclusive scan of H, so that X[p + 1] = new entries inserted at or before p
__global__ __launch_bounds__(256) void eu_place_base_kernel(const u32* __restrict__ col, const u64* __restrict__ vals, u32 nnz,
                                                           const u32* __restrict__ X, u32* __restrict__ out_col,
                                                           u64* __restrict__ out_val) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const u32 o = (u32)p + X[p + 1];
    out_col[o] = col[p];
    if (out_val) out_val[o] = vals[p];
}

// after the base: a new entry of the batch takes its place, a colliding one overwrites the value with MULTI_EDGE
__global__ __launch_bounds__(256) void eu_place_batch_kernel(const u32* __restrict__ col, const u64* __restrict__ vals, u32 nnz,
                                                            const u32* __restrict__ lb, const u32* __restrict__ N,
                                                            u32* __restrict__ out_col, u64* __restrict__ out_val) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= nnz) return;
    const u32 n0 = N[q], o = lb[q] + n0;
    if (N[q + 1] != n0) {
        out_col[o] = col[q];
        if (out_val) out_val[o] = vals[q];
    } else if (out_val) {
        out_val[o] = FGPU_MULTI_EDGE;
    }
}

// rp[r] = entries of the union before row r, r <= nrows
__global__ __launch_bounds__(256) void eu_rowptr_kernel(CsrView a, CsrView b, const u32* __restrict__ N, u64 nrows,
                                                       u32* __restrict__ rp) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    rp[r] = row_begin(a, (u32)r) + N[row_begin(b, (u32)r)];
}
__global__ __launch_bounds__(256) void eu_rowflag_kernel(const u32* __restrict__ rp, u64 nrows, u32* __restrict__ F) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    F[r] = (r < nrows && rp[r + 1] != rp[r]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void eu_rows_hyper_kernel(const u32* __restrict__ rp, const u32* __restrict__ F, u64 nrows,
                                                           u32 nvec_out, u32* __restrict__ rp_out, u32* __restrict__ hr_out) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    if (r == nrows) { rp_out[nvec_out] = rp[nrows]; return; }
    const u32 at = F[r];
    if (F[r + 1] == at) return;
    rp_out[at] = rp[r];
    hr_out[at] = (u32)r;
}

// the batch side of one union: where every entry of b meets a, and the scan of the new ones
struct EuSide {
    const fgpu_mat* a = nullptr;
    const fgpu_mat* b = nullptr;
    DevBuf<u32> wordrow;  // b's
    DevBuf<u32> lb, N;    // per entry of b; N has nnz + 1 entries
};

static fgpu_info eu_side_alloc(fgpu_ctx* ctx, EuSide& s, const fgpu_mat* a, const fgpu_mat* b) {
    s.a = a;
    s.b = b;
    FGPU_TRY(s.lb.alloc(ctx, b->nnz));
    FGPU_TRY(s.N.alloc(ctx, b->nnz + 1));
    if (b->nnz) return wordrow_build(ctx, b->rowptr, b->nvec, b->nnz, s.wordrow);
    FGPU_HIP(hipMemsetAsync(s.N.p, 0, sizeof(u32), ctx->stream()));
    return FGPU_OK;
}

// out = a U b with b's entries winning, placed by s.lb and s.N (scanned); n_new = s.N[b->nnz]
static fgpu_info eu_place(fgpu_ctx* ctx, const EuSide& s, u64 n_new, MatRef& out) {
    hipStream_t st = ctx->stream();
    const fgpu_mat *a = s.a, *b = s.b;
    const u64 nrows = a->nrows, nnz = a->nnz + n_new;
    const bool with_vals = a->vals != nullptr;
    DevBuf<u32> X, orp, F;
    FGPU_TRY(X.alloc(ctx, a->nnz + 2));
    FGPU_HIP(hipMemsetAsync(X.p, 0, (a->nnz + 2) * sizeof(u32), st));
    if (n_new) FGPU_TRY(launch(eu_hist_kernel, dim3(cdiv(b->nnz, 256)), dim3(256), 0, st, (const u32*)s.lb.p, (const u32*)s.N.p,
                               (u32)b->nnz, X.p));
    FGPU_TRY(scan_u32(ctx, X.p, X.p, a->nnz + 2, nullptr));
    FGPU_TRY(orp.alloc(ctx, nrows + 1));
    FGPU_TRY(launch(eu_rowptr_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, st, view_of(a), view_of(b), (const u32*)s.N.p, nrows,
                    orp.p));
    u32 nvec_out = 0;
    bool hyper = false;
    if (nrows > HYPER_MIN_ROWS) {
        DevBuf<u32> tot;
        FGPU_TRY(tot.alloc(ctx, 1));
        FGPU_TRY(F.alloc(ctx, nrows + 1));
        FGPU_TRY(launch(eu_rowflag_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, st, (const u32*)orp.p, nrows, F.p));
        FGPU_TRY(scan_u32(ctx, F.p, F.p, nrows + 1, tot.p));
        FGPU_TRY(read_u32(ctx, tot.p, &nvec_out));
        hyper = mat_prefer_hyper(nrows, nvec_out);
    }
    FGPU_TRY(mat_alloc(ctx, &out.m, nrows, a->ncols, nnz, with_vals, nvec_out, hyper));
    if (hyper) {
        FGPU_TRY(launch(eu_rows_hyper_kernel, dim3(cdiv(nrows + 1, 256)), dim3(256), 0, st, (const u32*)orp.p, (const u32*)F.p, nrows,
                        nvec_out, out->rowptr, out->hrows));
    } else {
        FGPU_HIP(hipMemcpyAsync(out->rowptr, orp.p, (nrows + 1) * sizeof(u32), hipMemcpyDeviceToDevice, st));
    }
    ProfScope prof(ctx, "eu_place", (a->nnz + b->nnz) * (with_vals ? 28 : 12));
    if (a->nnz)
        FGPU_TRY(launch(eu_place_base_kernel, dim3(cdiv(a->nnz, 256)), dim3(256), 0, st, (const u32*)a->colidx, (const u64*)a->vals,
                        (u32)a->nnz, (const u32*)X.p, out->colidx, out->vals));
    if (b->nnz)
        FGPU_TRY(launch(eu_place_batch_kernel, dim3(cdiv(b->nnz, 256)), dim3(256), 0, st, (const u32*)b->colidx, (const u64*)b->vals,
                        (u32)b->nnz, (const u32*)s.lb.p, (const u32*)s.N.p, out->colidx, out->vals));
    return FGPU_OK;
}

static fgpu_info edges_union_impl(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const u64* a_key, const u64* a_off,
                                  const u64* a_ids, u64 n_a, const fgpu_mat* fwd, const fgpu_mat* bwd, const u64* b_key,
                                  const u64* b_off, const u64* b_ids, u64 n_b, fgpu_mat** m_out, fgpu_mat** mt_out, u64** o_key,
                                  u64** o_off, u64** o_ids, u64* n_o_out, u64* stats) {
    FGPU_REQUIRE(ctx && m && fwd && m_out && mt_out && o_key && o_off && o_ids && n_o_out, FGPU_NULL_POINTER,
                 "fgpu_edges_union: NULL argument");
    *m_out = *mt_out = nullptr;
    *o_key = *o_off = *o_ids = nullptr;
    *n_o_out = 0;
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(n_a == 0 || (a_key && a_off && a_ids), FGPU_NULL_POINTER, "fgpu_edges_union: NULL a rows");
    FGPU_REQUIRE(n_b == 0 || (b_key && b_off && b_ids), FGPU_NULL_POINTER, "fgpu_edges_union: NULL b rows");
    FGPU_REQUIRE(m->vals, FGPU_INVALID, "fgpu_edges_union: m must be the tensor's UINT64 base (got a BOOL matrix)");
    FGPU_REQUIRE(fwd->vals, FGPU_INVALID, "fgpu_edges_union: fwd must be the batch's UINT64 matrix (got a BOOL matrix)");
    FGPU_REQUIRE(fwd->nrows == m->nrows && fwd->ncols == m->ncols, FGPU_INVALID,
                 "fgpu_edges_union: fwd is %llu x %llu, m is %llu x %llu", (unsigned long long)fwd->nrows,
                 (unsigned long long)fwd->ncols, (unsigned long long)m->nrows, (unsigned long long)m->ncols);
    FGPU_TRY(require_pattern_of("fgpu_edges_union", "mt", mt, m));
    FGPU_TRY(require_pattern_of("fgpu_edges_union", "bwd", bwd, m));
    FGPU_REQUIRE(n_a < 0xFFFFFFFFull && n_b < 0xFFFFFFFFull, FGPU_INVALID,
                 "fgpu_edges_union: %llu + %llu rows exceed the 32-bit position space", (unsigned long long)n_a,
                 (unsigned long long)n_b);
    MultiRows da, db;
    FGPU_TRY(da.check("fgpu_edges_union", "a", a_key, a_off, a_ids, n_a));
    FGPU_TRY(db.check("fgpu_edges_union", "b", b_key, b_off, b_ids, n_b));
    const u64 nf = fwd->nnz;
    FGPU_REQUIRE(m->nnz + nf < 0xFFFFFFFFull && mt->nnz + bwd->nnz < 0xFFFFFFFFull, FGPU_INVALID,
                 "fgpu_edges_union: %llu + %llu entries exceed the 32-bit position space", (unsigned long long)m->nnz,
                 (unsigned long long)nf);
    // every out row is at most a row of a or one inline id, plus a row of b or one inline id
    FGPU_REQUIRE(da.total() + db.total() + 2 * nf < 0xFFFFFFFFull, FGPU_INVALID,
                 "fgpu_edges_union: the merged ids may reach 2^32 - 1, the limit of the 32-bit scans");
    hipStream_t st = ctx->stream();
    // ---- classify + scans -------------------------------------------------------------------------------------------------
    // [0] new pairs [1] colliding pairs [2] out ids [3] new entries of mt [4] promoted [5] extended [6] no a row [7] no b row
    // [8] ids on both sides [9] longest out row
    DevBuf<u32> tot, C, L, startA, lenA, startB;
    FGPU_TRY(tot.alloc(ctx, 10));
    FGPU_HIP(hipMemsetAsync(tot.p, 0, 10 * sizeof(u32), st));
    EuSide sf, sb;
    u32 h[8] = {0};
    if (nf) {
        FGPU_TRY(da.upload(ctx, "eu_h2d"));
        FGPU_TRY(db.upload(ctx, "eu_h2d"));
    }
    FGPU_TRY(eu_side_alloc(ctx, sf, m, fwd));
    FGPU_TRY(eu_side_alloc(ctx, sb, mt, bwd));
    if (nf) {
        FGPU_TRY(C.alloc(ctx, nf + 1));
        FGPU_TRY(L.alloc(ctx, nf + 1));
        FGPU_TRY(startA.alloc(ctx, nf));
        FGPU_TRY(lenA.alloc(ctx, nf));
        FGPU_TRY(startB.alloc(ctx, nf));
        {
            ProfScope prof(ctx, "eu_classify", nf * 40);   // (plus one 64-byte line per probe step: the searches are the cost)
            FGPU_TRY(launch(eu_classify_kernel, dim3(cdiv(nf + 1, 256)), dim3(256), 0, st, view_of(m), (const u64*)m->vals, view_of(fwd),
                            (const u64*)fwd->vals, (const u32*)sf.wordrow.p, (u32)nf, (const u64*)da.key.p, (const u32*)da.off.p,
                            (u32)n_a, (const u64*)db.key.p, (const u32*)db.off.p, (u32)n_b, sf.lb.p, sf.N.p, C.p, L.p, startA.p, lenA.p,
                            startB.p, tot.p + 4));
        }
        ProfScope prof(ctx, "eu_scans", nf * 24);
        FGPU_TRY(scan_u32(ctx, sf.N.p, sf.N.p, nf + 1, tot.p + 0));
        FGPU_TRY(scan_u32(ctx, C.p, C.p, nf + 1, tot.p + 1));
        FGPU_TRY(scan_u32(ctx, L.p, L.p, nf + 1, tot.p + 2));
    }
    if (bwd->nnz) {
        ProfScope prof(ctx, "eu_locate_t", bwd->nnz * 16);
        FGPU_TRY(launch(eu_locate_kernel, dim3(cdiv(bwd->nnz + 1, 256)), dim3(256), 0, st, view_of(mt), view_of(bwd),
                        (const u32*)sb.wordrow.p, (u32)bwd->nnz, sb.lb.p, sb.N.p));
        FGPU_TRY(scan_u32(ctx, sb.N.p, sb.N.p, bwd->nnz + 1, tot.p + 3));
    }
    if (nf || bwd->nnz) FGPU_TRY(read_words(ctx, tot.p, 8, h));
    FGPU_REQUIRE(h[6] == 0, FGPU_INVALID,
                 "fgpu_edges_union: %u pairs of the batch hold MULTI_EDGE in m, and no a row was supplied for them", h[6]);
    FGPU_REQUIRE(h[7] == 0, FGPU_INVALID,
                 "fgpu_edges_union: %u colliding pairs hold MULTI_EDGE in fwd, and no b row was supplied for them", h[7]);
    const u64 n_new = h[0], n_o = h[1], total = h[2], n_new_t = h[3];
    // ---- the out rows, into scratch: an id on both sides fails the call before any output exists ---------------------------------
    DevBuf<u32> rowq, ooff, idrow;
    DevBuf<u64> okey, oids;
    u32 h2[2] = {0, 0};
    FGPU_TRY(ooff.alloc(ctx, n_o + 1));
    if (n_o) {
        FGPU_TRY(rowq.alloc(ctx, n_o));
        FGPU_TRY(okey.alloc(ctx, n_o));
        FGPU_TRY(oids.alloc(ctx, total));
        ProfScope prof(ctx, "eu_ids", nf * 12 + total * 24);
        FGPU_TRY(launch(eu_rows_kernel, dim3(cdiv(nf, 256)), dim3(256), 0, st, view_of(fwd), (const u32*)sf.wordrow.p, (u32)nf,
                        (const u32*)C.p, (const u32*)L.p, (u32)n_o, rowq.p, okey.p, ooff.p, tot.p + 9));
        FGPU_TRY(wordrow_build(ctx, ooff.p, (u32)n_o, total, idrow));
        FGPU_TRY(launch(eu_ids_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, (const u32*)ooff.p, (const u32*)idrow.p, (u32)total,
                        (const u32*)rowq.p, (const u32*)startA.p, (const u32*)lenA.p, (const u32*)startB.p, (const u64*)m->vals,
                        (const u64*)da.ids.p, (const u64*)fwd->vals, (const u64*)db.ids.p, oids.p, tot.p + 8));
        FGPU_TRY(read_words(ctx, tot.p + 8, 2, h2));
        FGPU_REQUIRE(h2[0] == 0, FGPU_INVALID,
                     "fgpu_edges_union: %u ids of the batch are already stored on their pair (an id on both sides of a colliding pair)",
                     h2[0]);
    } else {
        FGPU_HIP(hipMemsetAsync(ooff.p, 0, sizeof(u32), st));
    }
    // ---- outputs ----------------------------------------------------------------------------------------------------------
    ResultBuf rk, ro, ri;
    FGPU_REQUIRE(ro.alloc(ctx, (n_o + 1) * sizeof(u64)), FGPU_OOM, "fgpu_edges_union: out of host memory");
    if (n_o)
        FGPU_REQUIRE(rk.alloc(ctx, n_o * sizeof(u64)) && ri.alloc(ctx, total * sizeof(u64)), FGPU_OOM,
                     "fgpu_edges_union: out of host memory");
    MatRef om, ot;
    FGPU_TRY(eu_place(ctx, sf, n_new, om));
    FGPU_TRY(eu_place(ctx, sb, n_new_t, ot));
    {
        ProfScope prof(ctx, "eu_readback", n_o * 16 + total * 8);
        FGPU_TRY(ctx->d2h_widen((u64*)ro.p, ooff.p, n_o + 1));
        if (n_o) {
            FGPU_TRY(ctx->d2h(rk.p, okey.p, n_o * sizeof(u64)));
            FGPU_TRY(ctx->d2h(ri.p, oids.p, total * sizeof(u64)));
        }
    }
    if (stats) {
        stats[0] = n_new;
        stats[1] = n_o;
        stats[2] = h[4];
        stats[3] = h[5];
        stats[4] = total;
        stats[5] = h2[1];
        stats[6] = om->nnz;
        stats[7] = ot->nnz;
    }
    *m_out = om.release();
    *mt_out = ot.release();
    *o_key = (u64*)rk.release();
    *o_off = (u64*)ro.release();
    *o_ids = (u64*)ri.release();
    *n_o_out = n_o;
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_edges_union(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* mt, const uint64_t* a_key,
                                      const uint64_t* a_off, const uint64_t* a_ids, uint64_t n_a, const fgpu_mat* fwd,
                                      const fgpu_mat* bwd, const uint64_t* b_key, const uint64_t* b_off, const uint64_t* b_ids,
                                      uint64_t n_b, fgpu_mat** m_out, fgpu_mat** mt_out, uint64_t** o_key, uint64_t** o_off,
                                      uint64_t** o_ids, uint64_t* n_o, uint64_t stats[8]) {
    return published(ctx, edges_union_impl(ctx, m, mt, a_key, a_off, a_ids, n_a, fwd, bwd, b_key, b_off, b_ids, n_b, m_out, mt_out, o_key,
                                           o_off, o_ids, n_o, stats));
}
