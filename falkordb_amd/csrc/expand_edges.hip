// expand_edges.hip — fgpu_multi (a tensor's multi-edge rows resident on the device) and fgpu_expand_edges: the per-row path of
// CondTraverse (cond_traverse.rs:758-1117: expand_row + process_pairs) for a whole batch, the relationship emitted.  The
// reference walks one matrix row per input row and asks Tensor::get per pair and type; here one call gives the four columns
// (row, from, to, edge id) in the reference's order:
//
//   segments  a lane per (row, pass, type, layer): which stored run the pass walks — the row of the matrix source in m / dp, cut
//             to one entry by a binary search when the destination is bound too, or the row of the matrix destination in
//             mt_m / mt_dp when only that is bound — and its length.  S = exclusive scan of the lengths
//   gather    a lane per walked entry, its segment recovered through the wordrow index over S (bulk.hpp): the pair's matrix
//             coordinates, the dp shadow and the dm tombstone by binary search, for an incoming entry the forward value at
//             (src, bound); the self-loop, label-bitmap and first-only filters; count = 1, or the length of the table row under
//             FGPU_MULTI_EDGE (a pair without a row is counted, nothing is emitted for it)
//   order     the reference's order is the key order (row, pass, other node, type position).  One type without a dp layer: the
//             entry positions are that order already.  Otherwise the engine's stable sort (transpose.hip) on the items
//   place     O = exclusive scan of the counts in that order; a lane per output id finds its item through the wordrow index
//             over O and reads the inline id, or its id of the table row
//
// The only atomics are counters that place nothing.  No wavefront per row: a hub row is as many lanes as it has entries.
#include "edge_layers.hpp"

namespace fgpu {

struct EeBatch {
    const u32 *from, *to;      // k each, ~0u = unbound
    const EeType* ty;          // T
    const u64 *fbm, *tbm;      // nullable
    u32 k, P, T, L, flags;     // passes, types, layers (1: m only, 2: m and dp)
};
// what one segment (or one entry of it) walks
struct EeWalk {
    u32 i, p, t, l, msrc, mdst;
    bool rev;                  // the pair is oriented against storage: from_node is the matrix destination
};
__device__ __forceinline__ EeWalk ee_walk(const EeBatch& b, u32 s) {
    EeWalk w;
    w.l = s % b.L; s /= b.L;
    w.t = s % b.T; s /= b.T;
    w.p = s % b.P;
    w.i = s / b.P;
    const bool transposed = b.flags & FGPU_EDGES_TRANSPOSED;
    w.rev = w.p == 0 ? transposed : !transposed;
    const u32 f = b.from[w.i], t = b.to[w.i];
    w.msrc = w.rev ? t : f;
    w.mdst = w.rev ? f : t;
    return w;
}
// seg_b[s] = first position of the run, seg_len[s] = its length (seg_len[nseg] = 0, so that the scan ends in the total)
__global__ __launch_bounds__(256) void ee_segment_kernel(EeBatch b, u32 nseg, u32* __restrict__ seg_b, u32* __restrict__ seg_len,
                                                        u64* __restrict__ total) {
    const u64 s64 = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 len = 0;
    if (s64 < nseg) {
        const u32 s = (u32)s64;
        const EeWalk w = ee_walk(b, s);
        const EeType& y = b.ty[w.t];
        u32 beg = 0, end = 0;
        if (w.msrc != ~0u) {
            const CsrView& a = w.l ? y.dp : y.m;
            row_range(a, w.msrc, beg, end);
            if (w.mdst != ~0u) {
                const u32 q = find(a.colidx, beg, end, w.mdst);
                beg = q == ~0u ? 0u : q;
                end = q == ~0u ? 0u : q + 1;
            }
        } else if (w.mdst != ~0u) {
            row_range(w.l ? y.tdp : y.tm, w.mdst, beg, end);
        }
        len = end - beg;
        seg_b[s] = beg;
        seg_len[s] = len;
    } else if (s64 == nseg) {
        seg_len[nseg] = 0u;
    }
    ee_add(len, total);
}

// cnt: [0] pairs that hold MULTI_EDGE without a table row [1] entries walked outgoing [2] incoming [3] multi-edge pairs expanded
// [4] longest list [5] items that emit.  Item e: it_rp = row * P + pass, it_other = the node the walk varies, it_from / it_to the
// oriented pair, it_val = the inline id, or the start of the table row when it_ty has bit 31 set; it_ty & 63 = the type position
__global__ __launch_bounds__(256) void ee_gather_kernel(EeBatch b, const u32* __restrict__ seg_b, const u32* __restrict__ seg_off,
                                                       u32 nseg, const u32* __restrict__ wordrow, u32 n_ent, u32* __restrict__ it_rp,
                                                       u32* __restrict__ it_other, u32* __restrict__ it_from, u32* __restrict__ it_to,
                                                       u64* __restrict__ it_val, u32* __restrict__ it_ty, u32* __restrict__ it_cnt,
                                                       u64* __restrict__ total, u32* __restrict__ cnt) {
    const u64 e64 = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool live = e64 < n_ent;
    bool outw = false, missing = false, multi = false, valid = false;
    u32 c = 0;
    if (live) {
        const u32 e = (u32)e64;
        const u32 s = entry_vec(seg_off, wordrow, e);
        const EeWalk w = ee_walk(b, s);
        const EeType& y = b.ty[w.t];
        const u32 q = seg_b[s] + (e - seg_off[s]);
        outw = w.msrc != ~0u;
        u32 ms, md;
        u64 v = 0;
        if (outw) {
            ms = w.msrc;
            md = (w.l ? y.dp : y.m).colidx[q];
            if (w.l) {
                v = y.dpval[q];
                valid = true;
            } else {
                valid = probe(y.dp, ms, md) == ~0u && probe(y.dm, ms, md) == ~0u;   // (a shadowed pair is the dp item's)
                v = y.mval[q];
            }
        } else {
            md = w.mdst;
            ms = (w.l ? y.tdp : y.tm).colidx[q];
            const bool hidden = probe(y.tdm, md, ms) != ~0u;
            valid = w.l ? (hidden || probe(y.tm, md, ms) == ~0u) : !hidden;   // (a pair in both layers is the base item's)
            if (valid) valid = ee_value(y, ms, md, v);
        }
        if (w.p == 1 && ms == md) valid = false;   // the reverse pass drops self-loops (:894-945)
        const u32 fn = w.rev ? md : ms, tn = w.rev ? ms : md;
        if (valid && b.fbm && !ee_bit(b.fbm, fn)) valid = false;
        if (valid && b.tbm && !ee_bit(b.tbm, tn)) valid = false;
        const bool first_only = b.flags & FGPU_EDGES_FIRST_ONLY;
        if (valid && first_only) {   // the pair's representative comes from the first type that holds it
            u64 other;
            for (u32 t = 0; t < w.t && valid; ++t) valid = !ee_value(b.ty[t], ms, md, other);
        }
        u32 tyw = w.t;
        if (valid) {
            c = 1;
            if (v == FGPU_MULTI_EDGE) {
                const u32 r = find(y.mkey, 0u, y.n_multi, ((u64)ms << 32) | md);
                if (r == ~0u) {
                    missing = true;
                    valid = false;
                    c = 0;
                } else {
                    multi = true;
                    const u32 mb = y.moff[r];
                    c = first_only ? 1u : y.moff[r + 1] - mb;
                    v = mb;
                    tyw |= 0x80000000u;
                    atomicMax(cnt + 4, c);
                }
            }
        }
        it_rp[e] = w.i * b.P + w.p;
        it_other[e] = outw ? md : ms;
        it_from[e] = fn;
        it_to[e] = tn;
        it_val[e] = v;
        it_ty[e] = tyw;
        it_cnt[e] = c;
    } else if (e64 == n_ent) {
        it_cnt[n_ent] = 0u;
    }
    ee_add(c, total);
    count_if(missing, cnt + 0);
    count_if(live && outw, cnt + 1);
    count_if(live && !outw, cnt + 2);
    count_if(multi, cnt + 3);
    count_if(valid && c != 0, cnt + 5);
}

// one key of (row, pass, other node) when the product of the two spaces fits the sort's key space
__global__ __launch_bounds__(256) void ee_key_kernel(const u32* __restrict__ it_rp, const u32* __restrict__ it_other, u32 n_ent, u32 n,
                                                    u32* __restrict__ key, u32* __restrict__ idx) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    key[e] = it_rp[e] * n + it_other[e];
    idx[e] = (u32)e;
}
__global__ __launch_bounds__(256) void ee_iota_kernel(u32 n_ent, u32* __restrict__ idx) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e < n_ent) idx[e] = (u32)e;
}
// out[j] = a[perm[j]] (out[n_ent] = 0)
__global__ __launch_bounds__(256) void ee_permute_kernel(const u32* __restrict__ a, const u32* __restrict__ perm, u32 n_ent,
                                                        u32* __restrict__ out) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j < n_ent) out[j] = a[perm[j]];
    else if (j == n_ent) out[n_ent] = 0u;
}

// output id o belongs to item j = the last one with off[j] <= o; perm (nullable) maps the ordered items to their entries
__global__ __launch_bounds__(256) void ee_fill_kernel(EeBatch b, const u32* __restrict__ off, const u32* __restrict__ wordrow,
                                                     const u32* __restrict__ perm, u32 n_out, const u32* __restrict__ it_rp,
                                                     const u32* __restrict__ it_from, const u32* __restrict__ it_to,
                                                     const u64* __restrict__ it_val, const u32* __restrict__ it_ty,
                                                     u32* __restrict__ out_row, u32* __restrict__ out_from, u32* __restrict__ out_to,
                                                     u64* __restrict__ out_id, uint8_t* __restrict__ out_pass) {
    const u64 o64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (o64 >= n_out) return;
    const u32 o = (u32)o64;
    const u32 j = entry_vec(off, wordrow, o);
    const u32 e = perm ? perm[j] : j;
    const u32 tyw = it_ty[e];
    const u64 v = it_val[e];
    const u32 rp = it_rp[e];
    out_row[o] = rp / b.P;
    if (out_pass) out_pass[o] = (uint8_t)(rp % b.P);
    out_from[o] = it_from[e];
    out_to[o] = it_to[e];
    out_id[o] = (tyw & 0x80000000u) ? b.ty[tyw & 63u].mids[(u32)v + (o - off[j])] : v;
}

static fgpu_info expand_edges_impl(fgpu_ctx* ctx, const u64* from, const u64* to, u64 k, const fgpu_mat* const* m,
                                   const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                                   const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                                   int n_types, int flags, const u64* from_bitmap, const u64* to_bitmap, u32** out_row, u32** out_from,
                                   u32** out_to, u64** out_id, uint8_t** out_pass, u64* out_n, u64* stats) {
    const char* fn = "fgpu_expand_edges";
    FGPU_REQUIRE(ctx && out_row && out_from && out_to && out_id && out_n, FGPU_NULL_POINTER, "%s: NULL argument", fn);
    *out_row = *out_from = *out_to = nullptr;
    *out_id = nullptr;
    if (out_pass) *out_pass = nullptr;
    *out_n = 0;
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(k == 0 || (from && to), FGPU_NULL_POINTER, "%s: NULL from / to", fn);
    FGPU_REQUIRE(n_types == 0 || m, FGPU_NULL_POINTER, "%s: NULL m", fn);
    FGPU_REQUIRE(k <= EE_MAX_ROWS, FGPU_INVALID, "%s: %llu rows in one batch (at most %llu)", fn, (unsigned long long)k,
                 (unsigned long long)EE_MAX_ROWS);
    FGPU_REQUIRE(n_types >= 0 && n_types <= EE_MAX_TYPES, FGPU_INVALID, "%s: %d types (at most %d)", fn, n_types, EE_MAX_TYPES);
    FGPU_REQUIRE((flags & ~7) == 0, FGPU_INVALID, "%s: unknown flag bits in %d", fn, flags);
    if (k == 0 || n_types == 0) return FGPU_OK;
    // ---- the layers ------------------------------------------------------------------------------------------------------
    u64 n = 0;
    bool any_dp = false;
    std::vector<EeType> hty;
    FGPU_TRY(ee_types(fn, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, hty, n, any_dp));
    // ---- the rows --------------------------------------------------------------------------------------------------------
    const bool transposed = flags & FGPU_EDGES_TRANSPOSED, bidir = flags & FGPU_EDGES_BIDIRECTIONAL;
    std::vector<u32> f32(k), t32(k);
    bool need_in = false;
    for (u64 i = 0; i < k; ++i) {
        const bool fb = from[i] != ~0ull, tb = to[i] != ~0ull;
        FGPU_REQUIRE((!fb || from[i] < n) && (!tb || to[i] < n), FGPU_INVALID, "%s: row %llu = (%llu, %llu) names a node at or past %llu",
                     fn, (unsigned long long)i, (unsigned long long)from[i], (unsigned long long)to[i], (unsigned long long)n);
        f32[i] = fb ? (u32)from[i] : ~0u;
        t32[i] = tb ? (u32)to[i] : ~0u;
        // the forward pass walks in when only its matrix destination is bound; the reverse pass swaps the endpoints
        const bool fwd_in = transposed ? (fb && !tb) : (tb && !fb), rev_in = transposed ? (tb && !fb) : (fb && !tb);
        need_in = need_in || fwd_in || (bidir && rev_in);
    }
    if (need_in)
        for (int t = 0; t < n_types; ++t)
            FGPU_REQUIRE(ee_at(mt_m, t), FGPU_INVALID, "%s: a row walks incoming entries and mt_m[%d] is missing", fn, t);
    EeBatch b;
    b.k = (u32)k;
    b.P = bidir ? 2u : 1u;
    b.T = (u32)n_types;
    b.L = any_dp ? 2u : 1u;
    b.flags = (u32)flags;
    const u64 nseg64 = k * b.P * b.T * b.L;
    FGPU_REQUIRE(nseg64 < (1ull << 31), FGPU_INVALID, "%s: %llu rows x %u passes x %d types x %u layers exceed 2^31 segments", fn,
                 (unsigned long long)k, b.P, n_types, b.L);
    const u32 nseg = (u32)nseg64;
    hipStream_t st = ctx->stream();
    // ---- segments --------------------------------------------------------------------------------------------------------
    DevBuf<u32> dfrom, dto, seg_b, seg_off, tot, wr_seg;
    DevBuf<EeType> dty;
    DevBuf<u64> dfbm, dtbm;
    const u64 words = (n + 63) / 64;
    FGPU_TRY(dfrom.alloc(ctx, k));
    FGPU_TRY(dto.alloc(ctx, k));
    FGPU_TRY(dty.alloc(ctx, (size_t)n_types));
    FGPU_TRY(seg_b.alloc(ctx, nseg));
    FGPU_TRY(seg_off.alloc(ctx, (size_t)nseg + 1));
    FGPU_TRY(tot.alloc(ctx, 16));   // [0..1] entries walked, [2..3] ids emitted (64-bit sums), [4..] ee_gather_kernel's cnt
    if (from_bitmap) FGPU_TRY(dfbm.alloc(ctx, words));
    if (to_bitmap) FGPU_TRY(dtbm.alloc(ctx, words));
    FGPU_HIP(hipMemsetAsync(tot.p, 0, 16 * sizeof(u32), st));
    {
        ProfScope up(ctx, "ee_h2d", k * 8 + (size_t)n_types * sizeof(EeType));
        FGPU_TRY(ctx->h2d(dfrom.p, f32.data(), k * sizeof(u32)));
        FGPU_TRY(ctx->h2d(dto.p, t32.data(), k * sizeof(u32)));
        FGPU_TRY(ctx->h2d(dty.p, hty.data(), (size_t)n_types * sizeof(EeType)));
        if (from_bitmap) FGPU_TRY(ctx->h2d(dfbm.p, from_bitmap, words * sizeof(u64)));
        if (to_bitmap) FGPU_TRY(ctx->h2d(dtbm.p, to_bitmap, words * sizeof(u64)));
    }
    b.from = dfrom.p;
    b.to = dto.p;
    b.ty = dty.p;
    b.fbm = from_bitmap ? dfbm.p : nullptr;
    b.tbm = to_bitmap ? dtbm.p : nullptr;
    {
        ProfScope prof(ctx, "ee_segments", (u64)nseg * 8);
        FGPU_TRY(launch(ee_segment_kernel, dim3(cdiv((u64)nseg + 1, 256)), dim3(256), 0, st, b, nseg, seg_b.p, seg_off.p, (u64*)tot.p));
    }
    u32 h[10];
    FGPU_TRY(read_words(ctx, tot.p, 2, h));
    const u64 n_ent64 = (u64)h[0] | ((u64)h[1] << 32);
    FGPU_REQUIRE(n_ent64 < 0xFFFFFFFFull, FGPU_INVALID, "%s: the batch walks %llu stored entries, past the 32-bit position space", fn,
                 (unsigned long long)n_ent64);
    const u32 n_ent = (u32)n_ent64;
    if (stats) stats[7] = nseg;
    if (n_ent == 0) return FGPU_OK;
    FGPU_TRY(scan_u32(ctx, seg_off.p, seg_off.p, (u64)nseg + 1, nullptr));
    FGPU_TRY(wordrow_build(ctx, seg_off.p, nseg, n_ent, wr_seg));
    // ---- items -----------------------------------------------------------------------------------------------------------
    DevBuf<u32> it_rp, it_other, it_from, it_to, it_ty, it_cnt;
    DevBuf<u64> it_val;
    FGPU_TRY(it_rp.alloc(ctx, n_ent));
    FGPU_TRY(it_other.alloc(ctx, n_ent));
    FGPU_TRY(it_from.alloc(ctx, n_ent));
    FGPU_TRY(it_to.alloc(ctx, n_ent));
    FGPU_TRY(it_ty.alloc(ctx, n_ent));
    FGPU_TRY(it_cnt.alloc(ctx, (size_t)n_ent + 1));
    FGPU_TRY(it_val.alloc(ctx, n_ent));
    {
        ProfScope prof(ctx, "ee_gather", (u64)n_ent * 40);   // (plus one 64-byte line per probe step: the searches are the cost)
        FGPU_TRY(launch(ee_gather_kernel, dim3(cdiv((u64)n_ent + 1, 256)), dim3(256), 0, st, b, (const u32*)seg_b.p, (const u32*)seg_off.p,
                        nseg, (const u32*)wr_seg.p, n_ent, it_rp.p, it_other.p, it_from.p, it_to.p, it_val.p, it_ty.p, it_cnt.p,
                        (u64*)(tot.p + 2), tot.p + 4));
    }
    // ---- order -----------------------------------------------------------------------------------------------------------
    // entry order is (row, pass, type, layer, other node); the reference's is (row, pass, other node, type) — the same with one
    // type and no dp layer.  Otherwise a stable sort by (row, pass, other node) keeps the types of a pair in scan order (at most
    // one layer of a type carries a live item of a pair)
    DevBuf<u32> perm, key, idx, keyptr, cnt_o;
    u64 path = 0;
    if (b.T > 1 || b.L > 1) {
        const u64 nrp = (u64)k * b.P;
        FGPU_TRY(perm.alloc(ctx, n_ent));
        FGPU_TRY(idx.alloc(ctx, n_ent));
        ProfScope prof(ctx, "ee_sort", (u64)n_ent * 32);
        if (nrp * n <= (1ull << 22)) {   // (the sort hands back a pointer per key: keep that array small)
            path = 1;
            FGPU_TRY(key.alloc(ctx, n_ent));
            FGPU_TRY(keyptr.alloc(ctx, nrp * n + 1));
            FGPU_TRY(launch(ee_key_kernel, dim3(cdiv(n_ent, 256)), dim3(256), 0, st, (const u32*)it_rp.p, (const u32*)it_other.p, n_ent,
                            (u32)n, key.p, idx.p));
            FGPU_TRY(sort_u32_pairs_by_key(ctx, key.p, idx.p, n_ent, nrp * n, perm.p, keyptr.p));
        } else {
            // least significant key first: by other node, then (stable) by (row, pass)
            path = 2;
            FGPU_TRY(key.alloc(ctx, (size_t)n_ent + 1));
            FGPU_TRY(keyptr.alloc(ctx, std::max(n, nrp) + 1));
            FGPU_TRY(launch(ee_iota_kernel, dim3(cdiv(n_ent, 256)), dim3(256), 0, st, n_ent, idx.p));
            FGPU_TRY(sort_u32_pairs_by_key(ctx, it_other.p, idx.p, n_ent, n, perm.p, keyptr.p));
            FGPU_TRY(launch(ee_permute_kernel, dim3(cdiv((u64)n_ent + 1, 256)), dim3(256), 0, st, (const u32*)it_rp.p, (const u32*)perm.p,
                            n_ent, key.p));
            FGPU_TRY(sort_u32_pairs_by_key(ctx, key.p, perm.p, n_ent, nrp, idx.p, keyptr.p));
            std::swap(perm, idx);
        }
        FGPU_TRY(cnt_o.alloc(ctx, (size_t)n_ent + 1));
        FGPU_TRY(launch(ee_permute_kernel, dim3(cdiv((u64)n_ent + 1, 256)), dim3(256), 0, st, (const u32*)it_cnt.p, (const u32*)perm.p, n_ent,
                        cnt_o.p));
    }
    // ---- place -----------------------------------------------------------------------------------------------------------
    FGPU_TRY(read_words(ctx, tot.p, 10, h));
    FGPU_REQUIRE(h[4] == 0, FGPU_INVALID, "%s: %u visited pairs hold MULTI_EDGE in a tensor, and its table has no row for them", fn, h[4]);
    const u64 n_out64 = (u64)h[2] | ((u64)h[3] << 32);
    FGPU_REQUIRE(n_out64 < 0xFFFFFFFFull, FGPU_INVALID, "%s: the batch emits %llu ids, past the 32-bit position space", fn,
                 (unsigned long long)n_out64);
    const u32 n_out = (u32)n_out64;
    if (stats) {
        stats[0] = h[5];
        stats[1] = h[6];
        stats[2] = n_out;
        stats[3] = h[7];
        stats[4] = n_out ? std::max(h[8], 1u) : 0u;
        stats[5] = path;
        stats[6] = h[9];
    }
    if (n_out == 0) return FGPU_OK;
    u32* off = perm.p ? cnt_o.p : it_cnt.p;
    DevBuf<u32> wr_out, o_row, o_from, o_to;
    DevBuf<u64> o_id;
    DevBuf<uint8_t> o_pass;
    FGPU_TRY(scan_u32(ctx, off, off, (u64)n_ent + 1, nullptr));
    FGPU_TRY(wordrow_build(ctx, off, n_ent, n_out, wr_out));
    FGPU_TRY(o_row.alloc(ctx, n_out));
    FGPU_TRY(o_from.alloc(ctx, n_out));
    FGPU_TRY(o_to.alloc(ctx, n_out));
    FGPU_TRY(o_id.alloc(ctx, n_out));
    if (out_pass) FGPU_TRY(o_pass.alloc(ctx, n_out));
    ResultBuf rr, rf, rt, ri, rp;
    FGPU_REQUIRE((!out_pass || rp.alloc(ctx, n_out)) && rr.alloc(ctx, (size_t)n_out * 4) && rf.alloc(ctx, (size_t)n_out * 4) && rt.alloc(ctx, (size_t)n_out * 4) &&
                     ri.alloc(ctx, (size_t)n_out * 8),
                 FGPU_OOM, "%s: out of host memory", fn);
    {
        ProfScope prof(ctx, "ee_fill", (u64)n_out * 24);
        FGPU_TRY(launch(ee_fill_kernel, dim3(cdiv(n_out, 256)), dim3(256), 0, st, b, (const u32*)off, (const u32*)wr_out.p,
                        (const u32*)perm.p, n_out, (const u32*)it_rp.p, (const u32*)it_from.p, (const u32*)it_to.p, (const u64*)it_val.p,
                        (const u32*)it_ty.p, o_row.p, o_from.p, o_to.p, o_id.p, o_pass.p));
    }
    {
        ProfScope prof(ctx, "ee_readback", (u64)n_out * 20);
        FGPU_TRY(ctx->d2h(rr.p, o_row.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(rf.p, o_from.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(rt.p, o_to.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(ri.p, o_id.p, (size_t)n_out * 8));
        if (out_pass) FGPU_TRY(ctx->d2h(rp.p, o_pass.p, n_out));
    }
    *out_row = (u32*)rr.release();
    *out_from = (u32*)rf.release();
    *out_to = (u32*)rt.release();
    *out_id = (u64*)ri.release();
    if (out_pass) *out_pass = (uint8_t*)rp.release();
    *out_n = n_out;
    return FGPU_OK;
}

static fgpu_info multi_new_impl(fgpu_ctx* ctx, const u64* key, const u64* off, const u64* ids, u64 n_multi, fgpu_multi** out) {
    FGPU_REQUIRE(ctx && out, FGPU_NULL_POINTER, "fgpu_multi_new: NULL argument");
    *out = nullptr;
    FGPU_REQUIRE(n_multi == 0 || (key && off && ids), FGPU_NULL_POINTER, "fgpu_multi_new: NULL row arrays");
    FGPU_REQUIRE(n_multi < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_multi_new: %llu rows exceed the 32-bit position space",
                 (unsigned long long)n_multi);
    MultiRows rows;
    FGPU_TRY(rows.check("fgpu_multi_new", "multi", key, off, ids, n_multi));
    for (u64 r = 0; r < n_multi; ++r)
        FGPU_REQUIRE((key[r] >> 32) < 0xFFFFFFFFull && (u32)key[r] != ~0u, FGPU_INVALID,
                     "fgpu_multi_new: key %llu names a node past the 32-bit id space", (unsigned long long)r);
    FGPU_TRY(rows.upload(ctx, "multi_h2d"));
    std::unique_ptr<fgpu_multi> t(new fgpu_multi());
    t->ctx = ctx;
    t->n = n_multi;
    t->total = rows.total();
    t->key = std::move(rows.key);
    t->ids = std::move(rows.ids);
    t->off = std::move(rows.off);
    *out = t.release();
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_multi_new(fgpu_ctx* ctx, const uint64_t* key, const uint64_t* off, const uint64_t* ids, uint64_t n_multi,
                                    fgpu_multi** out) {
    return published(ctx, multi_new_impl(ctx, key, off, ids, n_multi, out));
}

extern "C" fgpu_info fgpu_multi_free(fgpu_multi* t) {
    if (!t) return FGPU_OK;
    t->ctx->fence_lanes();   // as fgpu_mat_free: calls other lanes queued on the table finish before its blocks are reused
    delete t;
    return FGPU_OK;
}

extern "C" fgpu_info fgpu_multi_size(const fgpu_multi* t, uint64_t* n_multi, uint64_t* n_ids) {
    FGPU_REQUIRE(t, FGPU_NULL_POINTER, "fgpu_multi_size: NULL table");
    if (n_multi) *n_multi = t->n;
    if (n_ids) *n_ids = t->total;
    return FGPU_OK;
}

extern "C" fgpu_info fgpu_expand_edges(fgpu_ctx* ctx, const uint64_t* from, const uint64_t* to, uint64_t k, const fgpu_mat* const* m,
                                       const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                                       const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                                       int n_types, int flags, const uint64_t* from_bitmap, const uint64_t* to_bitmap,
                                       uint32_t** out_row, uint32_t** out_from, uint32_t** out_to, uint64_t** out_id, uint8_t** out_pass,
                                       uint64_t* out_n, uint64_t stats[8]) {
    return expand_edges_impl(ctx, from, to, k, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, flags, from_bitmap, to_bitmap, out_row,
                             out_from, out_to, out_id, out_pass, out_n, stats);
}
