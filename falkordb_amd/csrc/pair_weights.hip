// pair_weights.hip — fgpu_pair_weights: the weighted pair matrix algo.MSF (algo_procedures.rs:1403-1704), algo.SPpaths (:2156-2257,
// :2405-2514) and the hop-bounded pruning table start from.  One entry per ordered node pair: the smallest weight over the
// selected relationship types, their multi-edges and the traversal direction (W), and the relationship that was kept (K).  The
// reference walks every relationship on the host and folds it into a map keyed by pair; here one call reads the tensors' own
// layers (no fold is needed):
//
//   entries     a lane per stored entry of every type's m and dp, its layer found in the 2 T + 1 layer bases and its row through a
//               wordrow index built per call (bulk.hpp): an m entry checks the dp shadow and the dm tombstone by binary search;
//               self-loops and ends outside the active set leave here; count = 1, or the length of the table row under
//               FGPU_MULTI_EDGE (a pair without a row is counted, nothing is examined for it)
//   weights     R = exclusive scan of the counts; a lane per relationship finds its entry through the wordrow index over R, reads
//               the inline id or its id of the table row, and looks the attribute up by binary search (find of bulk.hpp).  NEGATE,
//               -0.0 -> +0.0, DROP_NONFINITE and REFUSE_NEGATIVE apply in that order; a refused id goes through an integer atomicMin
//   candidates  C = exclusive scan of the kept flags; a lane per kept relationship writes (from, to, key(weight), id) once per
//               direction
//   group       the candidate INDICES ordered by (from, to): two passes of the stable counting sort fgpu_edges_build uses
//               (transpose.hip; by `to`, then by `from` of the permuted order), in 16-bit digits past 2^31 candidates
//   reduce      a lane per sorted position: head = "pair differs from the predecessor", E = exclusive scan of the heads.  A run of
//               one writes its pair's (key, id) with plain stores; a longer run takes the minimum key with an integer atomicMin on
//               the pair's slot, and in a second pass the lanes that hold that key take the minimum id the same way.  Both minima
//               are functions of the candidate set alone: no floating-point atomic, nothing depends on launch order
//   emit        a lane per pair turns the key back into binary64 bits; the row pointers are a lane per row, a binary search for
//               the row's first sorted position, read through E
//
// No wavefront per row or per pair: a hub pair is as many lanes as it has candidates.
#include <algorithm>

#include "edge_layers.hpp"

namespace fgpu {

constexpr u64 PW_SIGN = 0x8000000000000000ull;
constexpr u64 PW_EXP = 0x7FF0000000000000ull;
constexpr u64 PW_ONE = 0x3FF0000000000000ull;

// the order of fgpu_msf: IEEE totalOrder of the bit pattern (-0.0 is +0.0 by the time a weight gets here)
__device__ __forceinline__ u64 pw_key(u64 bits) { return (bits >> 63) ? ~bits : bits ^ PW_SIGN; }
__device__ __forceinline__ u64 pw_bits(u64 key) { return (key >> 63) ? key ^ PW_SIGN : ~key; }

struct PwIn {
    const EeType* ty;          // T types
    const u32* lbase;          // 2 T + 1: entries before layer 2 t (m of type t) and 2 t + 1 (its dp)
    const u32* const* lwr;     // 2 T: the layer's wordrow index (nullptr for an empty layer)
    const u64* active;         // nullable
    u32 L;                     // 2 T
};

__global__ __launch_bounds__(256) void pw_attr_order_kernel(const u64* __restrict__ ids, u32 n_attr, u32* __restrict__ bad) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    count_if(k + 1 < n_attr && ids[k] >= ids[k + 1], bad);
}

// cnt: [0] pairs that hold MULTI_EDGE without a table row [1] pairs examined [2] multi-edge pairs expanded.  Entry e: its pair,
// ent_val = the inline id, or the start of the table row when ent_ty has bit 31 set; ent_ty & 63 = the type position
__global__ __launch_bounds__(256) void pw_entry_kernel(PwIn in, u32 n_ent, u32* __restrict__ ent_src, u32* __restrict__ ent_dst,
                                                      u64* __restrict__ ent_val, u32* __restrict__ ent_ty, u32* __restrict__ ent_cnt,
                                                      u64* __restrict__ total, u32* __restrict__ cnt) {
    const u64 e64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool missing = false, multi = false, valid = false;
    u32 c = 0;
    if (e64 < n_ent) {
        const u32 e = (u32)e64;
        const u32 l = row_of(in.lbase, 0u, in.L - 1u, e);
        const u32 t = l >> 1, q = e - in.lbase[l];
        const EeType& y = in.ty[t];
        const CsrView& a = (l & 1u) ? y.dp : y.m;
        const u32 s = entry_row(a, in.lwr[l], q), d = a.colidx[q];
        u64 v;
        if (l & 1u) {
            v = y.dpval[q];
            valid = true;
        } else {
            v = y.mval[q];
            valid = probe(y.dp, s, d) == ~0u && probe(y.dm, s, d) == ~0u;   // (a shadowed pair is the dp entry's)
        }
        if (s == d) valid = false;
        if (valid && in.active && !(ee_bit(in.active, s) && ee_bit(in.active, d))) valid = false;
        u32 tyw = t;
        if (valid) {
            c = 1;
            if (v == FGPU_MULTI_EDGE) {
                const u32 r = find(y.mkey, 0u, y.n_multi, ((u64)s << 32) | d);
                if (r == ~0u) {
                    missing = true;
                    valid = false;
                    c = 0;
                } else {
                    multi = true;
                    const u32 mb = y.moff[r];
                    c = y.moff[r + 1] - mb;
                    v = mb;
                    tyw |= 0x80000000u;
                }
            }
        }
        ent_src[e] = s;
        ent_dst[e] = d;
        ent_val[e] = v;
        ent_ty[e] = tyw;
        ent_cnt[e] = c;
    } else if (e64 == n_ent) {
        ent_cnt[n_ent] = 0u;
    }
    ee_add(c, total);
    count_if(missing, cnt + 0);
    count_if(valid, cnt + 1);
    count_if(multi, cnt + 2);
}

struct PwAttr {
    const u64* ids;            // nullptr: every relationship weighs 1.0
    const double* vals;
    u32 n;
    int flags;
    double missing;
};

// cnt: [0] dropped as non-finite [1] took `missing`.  rel_keep has n_rel + 1 entries (the last 0, so that the scan ends in the total)
__global__ __launch_bounds__(256) void pw_rel_kernel(PwIn in, PwAttr at, const u32* __restrict__ rel_off, const u32* __restrict__ wordrow,
                                                    u32 n_rel, const u64* __restrict__ ent_val, const u32* __restrict__ ent_ty,
                                                    u64* __restrict__ rel_key, u64* __restrict__ rel_id, u32* __restrict__ rel_ent,
                                                    u32* __restrict__ rel_keep, u64* __restrict__ refused, u32* __restrict__ cnt) {
    const u64 r64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool dropped = false, took = false;
    if (r64 < n_rel) {
        const u32 r = (u32)r64;
        const u32 e = entry_vec(rel_off, wordrow, r);
        const u32 tyw = ent_ty[e];
        const u64 v = ent_val[e];
        const u64 id = (tyw & 0x80000000u) ? in.ty[tyw & 63u].mids[(u32)v + (r - rel_off[e])] : v;
        u64 bits = PW_ONE;
        bool keep = true;
        if (at.ids) {
            const u32 k = find(at.ids, 0u, at.n, id);
            took = k == ~0u;
            double w = took ? at.missing : at.vals[k];
            if (!took && (at.flags & FGPU_PAIRS_NEGATE)) w = -w;
            bits = (u64)__double_as_longlong(w);
            if (bits == PW_SIGN) bits = 0;
            const bool nonfinite = (bits & PW_EXP) == PW_EXP;
            if (nonfinite && (at.flags & FGPU_PAIRS_DROP_NONFINITE)) {
                dropped = true;
                keep = false;
            } else if (!nonfinite && (bits >> 63) && (at.flags & FGPU_PAIRS_REFUSE_NEGATIVE)) {
                atomicMin((unsigned long long*)refused, (unsigned long long)id);
            }
        }
        rel_key[r] = pw_key(bits);
        rel_id[r] = id;
        rel_ent[r] = e;
        rel_keep[r] = keep ? 1u : 0u;
    } else if (r64 == n_rel) {
        rel_keep[n_rel] = 0u;
    }
    count_if(dropped, cnt + 0);
    count_if(took, cnt + 1);
}

// pos = the exclusive scan of rel_keep (n_rel + 1 entries); D candidates per kept relationship
__global__ __launch_bounds__(256) void pw_place_kernel(const u32* __restrict__ pos, u32 n_rel, int flags, const u32* __restrict__ rel_ent,
                                                      const u64* __restrict__ rel_key, const u64* __restrict__ rel_id,
                                                      const u32* __restrict__ ent_src, const u32* __restrict__ ent_dst,
                                                      u32* __restrict__ c_from, u32* __restrict__ c_to, u64* __restrict__ c_key,
                                                      u64* __restrict__ c_id) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rel) return;
    const u32 p0 = pos[r];
    if (pos[r + 1] == p0) return;
    const u32 e = rel_ent[r], s = ent_src[e], d = ent_dst[e];
    const u64 key = rel_key[r], id = rel_id[r];
    const bool both = (flags & (FGPU_PAIRS_OUT | FGPU_PAIRS_IN)) == (FGPU_PAIRS_OUT | FGPU_PAIRS_IN);
    u32 p = both ? 2u * p0 : p0;
    if (flags & FGPU_PAIRS_OUT) {
        c_from[p] = s; c_to[p] = d; c_key[p] = key; c_id[p] = id;
        ++p;
    }
    if (flags & FGPU_PAIRS_IN) {
        c_from[p] = d; c_to[p] = s; c_key[p] = key; c_id[p] = id;
    }
}

__global__ __launch_bounds__(256) void pw_iota_kernel(u32* __restrict__ v, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = (u32)i;
}
// the next pass's keys: a digit of the coordinate of the candidate at every position of the order so far
__global__ __launch_bounds__(256) void pw_digit_kernel(const u32* __restrict__ coord, const u32* __restrict__ perm, u64 n, u32 shift,
                                                      u32 mask, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (coord[perm[i]] >> shift) & mask;
}
// one stable pass: perm_out = perm_in reordered by coord[perm_in[.]] (< nkeys)
static fgpu_info pw_sort_pass(fgpu_ctx* ctx, const u32* coord, const u32* perm_in, u64 n, u64 nkeys, u32* keys, u32* perm_out) {
    hipStream_t st = ctx->stream();
    const dim3 grid(cdiv(n, 256));
    DevBuf<u32> keyptr;
    if (nkeys <= (1ull << 31)) {
        FGPU_TRY(launch(pw_digit_kernel, grid, dim3(256), 0, st, coord, perm_in, n, 0u, 0xFFFFFFFFu, keys));
        FGPU_TRY(keyptr.alloc(ctx, nkeys + 1));
        const fgpu_info i = sort_u32_pairs_stable(ctx, keys, perm_in, n, nkeys, perm_out, keyptr.p);
        if (i != FGPU_NO_VALUE) return i;
        return sort_u32_pairs_by_key(ctx, keys, perm_in, n, nkeys, perm_out, keyptr.p);
    }
    // a key space past 2^31: the same stable sort, least significant 16 bits first
    FGPU_TRY(keyptr.alloc(ctx, 65536 + 1));
    DevBuf<u32> mid;
    FGPU_TRY(mid.alloc(ctx, n));
    FGPU_TRY(launch(pw_digit_kernel, grid, dim3(256), 0, st, coord, perm_in, n, 0u, 0xFFFFu, keys));
    FGPU_TRY(sort_u32_pairs_by_key(ctx, keys, perm_in, n, 65536, mid.p, keyptr.p));
    FGPU_TRY(launch(pw_digit_kernel, grid, dim3(256), 0, st, coord, (const u32*)mid.p, n, 16u, 0xFFFFu, keys));
    return sort_u32_pairs_by_key(ctx, keys, mid.p, n, 65536, perm_out, keyptr.p);
}

// the candidates in (from, to) order, and head[i] = first candidate of its pair
__global__ __launch_bounds__(256) void pw_sorted_kernel(const u32* __restrict__ c_from, const u32* __restrict__ c_to,
                                                       const u64* __restrict__ c_key, const u64* __restrict__ c_id,
                                                       const u32* __restrict__ perm, u64 n, u64* __restrict__ s_pair,
                                                       u64* __restrict__ s_key, u64* __restrict__ s_id) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 t = perm[i];
    s_pair[i] = ((u64)c_from[t] << 32) | c_to[t];
    s_key[i] = c_key[t];
    s_id[i] = c_id[t];
}
__global__ __launch_bounds__(256) void pw_head_kernel(const u64* __restrict__ s_pair, u64 n, u32* __restrict__ head) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) head[i] = (i == 0 || s_pair[i - 1] != s_pair[i]) ? 1u : 0u;
}

// E = the exclusive scan of head.  min_key / min_id arrive filled with ~0; start[p] = first position of pair p, start[n_pairs] = n
__global__ __launch_bounds__(256) void pw_min_key_kernel(const u64* __restrict__ s_pair, const u64* __restrict__ s_key,
                                                        const u64* __restrict__ s_id, const u32* __restrict__ E, u64 n, u32 n_pairs,
                                                        u32* __restrict__ colidx, u32* __restrict__ start, u64* __restrict__ min_key,
                                                        u64* __restrict__ min_id) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) start[n_pairs] = (u32)n;
    const u64 k = s_pair[i];
    const bool h = i == 0 || s_pair[i - 1] != k;
    const bool last = i + 1 == n || s_pair[i + 1] != k;
    const u32 p = h ? E[i] : E[i] - 1u;   // (a run's head lies before its other positions: E counts it there)
    if (h) {
        colidx[p] = (u32)k;
        start[p] = (u32)i;
    }
    if (h && last) {
        min_key[p] = s_key[i];
        min_id[p] = s_id[i];
    } else {
        atomicMin((unsigned long long*)(min_key + p), (unsigned long long)s_key[i]);
    }
}
__global__ __launch_bounds__(256) void pw_min_id_kernel(const u64* __restrict__ s_pair, const u64* __restrict__ s_key,
                                                       const u64* __restrict__ s_id, const u32* __restrict__ E, u64 n,
                                                       const u64* __restrict__ min_key, u64* __restrict__ min_id) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = s_pair[i];
    const bool h = i == 0 || s_pair[i - 1] != k;
    const bool last = i + 1 == n || s_pair[i + 1] != k;
    if (h && last) return;
    const u32 p = h ? E[i] : E[i] - 1u;   // (a run's head lies before its other positions: E counts it there)
    if (s_key[i] == min_key[p]) atomicMin((unsigned long long*)(min_id + p), (unsigned long long)s_id[i]);
}
// wvals / kvals nullable; *longest = most candidates of one pair
__global__ __launch_bounds__(256) void pw_emit_kernel(const u64* __restrict__ min_key, const u64* __restrict__ min_id,
                                                     const u32* __restrict__ start, u32 n_pairs, u64* __restrict__ wvals,
                                                     u64* __restrict__ kvals, u32* __restrict__ longest) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 len = 0;
    if (p < n_pairs) {
        if (wvals) wvals[p] = pw_bits(min_key[p]);
        if (kvals) kvals[p] = min_id[p];
        len = start[p + 1] - start[p];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u32 o = __shfl_xor(len, d, WAVE); len = o > len ? o : len; }
    if (lane_id() == 0 && len) atomicMax(longest, len);
}
// rowptr[r] = pairs before row r: the pair of the first sorted position whose `from` is >= r
__global__ __launch_bounds__(256) void pw_rowptr_kernel(const u64* __restrict__ s_pair, u64 n, const u32* __restrict__ E, u32 n_pairs,
                                                       u64 nrows, u32* __restrict__ rowptr) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    const u32 lo = lower_bound(s_pair, 0u, (u32)n, r << 32);
    rowptr[r] = lo < n ? E[lo] : n_pairs;
}

static fgpu_info pw_empty(fgpu_ctx* ctx, fgpu_mat** out, u64 n, bool with_vals) {
    MatRef m;
    FGPU_TRY(mat_alloc(ctx, &m.m, n, n, 0, with_vals, 0, true));
    FGPU_HIP(hipMemsetAsync(m->rowptr, 0, sizeof(u32), ctx->stream()));
    FGPU_TRY(mat_finalize(m.get()));
    *out = m.release();
    return FGPU_OK;
}

static fgpu_info pair_weights_impl(fgpu_ctx* ctx, const fgpu_mat* const* m_in, const fgpu_mat* const* dp_in, const fgpu_mat* const* dm_in,
                                   const fgpu_multi* const* multi_in, int n_types_in, int flags, const u64* active_bitmap,
                                   const u64* attr_ids, const double* attr_vals, u64 n_attr, double missing, fgpu_mat** W_out,
                                   fgpu_mat** K_out, u64* refused_id, u64* stats) {
    const char* fn = "fgpu_pair_weights";
    FGPU_REQUIRE(ctx, FGPU_NULL_POINTER, "%s: NULL context", fn);
    if (stats) memset(stats, 0, 8 * sizeof(u64));
    FGPU_REQUIRE(n_types_in > 0 && n_types_in <= EE_MAX_TYPES, FGPU_INVALID, "%s: %d types (1 to %d)", fn, n_types_in, EE_MAX_TYPES);
    FGPU_REQUIRE(m_in, FGPU_NULL_POINTER, "%s: NULL m", fn);
    const int known = FGPU_PAIRS_OUT | FGPU_PAIRS_IN | FGPU_PAIRS_NEGATE | FGPU_PAIRS_DROP_NONFINITE | FGPU_PAIRS_REFUSE_NEGATIVE;
    FGPU_REQUIRE((flags & ~known) == 0, FGPU_INVALID, "%s: unknown flag bits in %d", fn, flags);
    FGPU_REQUIRE(flags & (FGPU_PAIRS_OUT | FGPU_PAIRS_IN), FGPU_INVALID, "%s: neither FGPU_PAIRS_OUT nor FGPU_PAIRS_IN is set", fn);
    FGPU_REQUIRE(!attr_ids || n_attr == 0 || attr_vals, FGPU_NULL_POINTER, "%s: attr_ids without attr_vals", fn);
    FGPU_REQUIRE(n_attr < 0xFFFFFFFFull, FGPU_INVALID, "%s: %llu attribute values exceed the 32-bit position space", fn,
                 (unsigned long long)n_attr);
    // ---- the layers; a type given twice is one type ------------------------------------------------------------------------
    std::vector<const fgpu_mat*> vm, vdp, vdm;
    std::vector<const fgpu_multi*> vmu;
    for (int t = 0; t < n_types_in; ++t) {
        const fgpu_mat *a = m_in[t], *b = ee_at(dp_in, t), *c = ee_at(dm_in, t);
        const fgpu_multi* u = multi_in ? multi_in[t] : nullptr;
        bool seen = false;
        for (size_t s = 0; s < vm.size() && !seen; ++s) seen = a && vm[s] == a && vdp[s] == b && vdm[s] == c && vmu[s] == u;
        if (seen) continue;
        vm.push_back(a); vdp.push_back(b); vdm.push_back(c); vmu.push_back(u);
    }
    const int T = (int)vm.size();
    u64 n = 0;
    bool any_dp = false;
    std::vector<EeType> hty;
    FGPU_TRY(ee_types(fn, vm.data(), vdp.data(), vdm.data(), nullptr, nullptr, nullptr, vmu.data(), T, hty, n, any_dp));
    const bool unit = attr_ids == nullptr;
    const bool both = (flags & (FGPU_PAIRS_OUT | FGPU_PAIRS_IN)) == (FGPU_PAIRS_OUT | FGPU_PAIRS_IN);
    const u32 L = 2u * (u32)T;
    std::vector<u32> lbase(L + 1, 0u);
    u64 n_ent64 = 0;
    for (u32 l = 0; l < L; ++l) {
        lbase[l] = (u32)n_ent64;
        const fgpu_mat* a = (l & 1u) ? vdp[l >> 1] : vm[l >> 1];
        n_ent64 += a ? a->nnz : 0;
        FGPU_REQUIRE(n_ent64 < 0xFFFFFFFFull, FGPU_INVALID, "%s: the layers hold %llu stored entries or more, past the 32-bit position space",
                     fn, (unsigned long long)n_ent64);
    }
    lbase[L] = (u32)n_ent64;
    const u32 n_ent = (u32)n_ent64;
    hipStream_t st = ctx->stream();
    auto finish_empty = [&]() -> fgpu_info {
        MatRef w, k;
        if (W_out) FGPU_TRY(pw_empty(ctx, &w.m, n, !unit));
        if (K_out) FGPU_TRY(pw_empty(ctx, &k.m, n, true));
        if (W_out) *W_out = w.release();
        if (K_out) *K_out = k.release();
        return FGPU_OK;
    };
    // ---- the attribute list ------------------------------------------------------------------------------------------------
    DevBuf<u32> tot;
    DevBuf<u64> d_attr_ids, d_refused;
    DevBuf<double> d_attr_vals;
    FGPU_TRY(tot.alloc(ctx, 16));   // [0..1] relationships (64-bit sum) [2] attr pairs out of order [3..5] pw_entry_kernel's cnt
                                    // [6..7] pw_rel_kernel's cnt [8] kept relationships [9] pairs [10] most candidates of one pair
    FGPU_TRY(d_refused.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(tot.p, 0, 16 * sizeof(u32), st));
    FGPU_HIP(hipMemsetAsync(d_refused.p, 0xFF, sizeof(u64), st));
    if (!unit && n_attr) {
        ProfScope up(ctx, "pw_h2d", n_attr * 16);
        FGPU_TRY(d_attr_ids.alloc(ctx, n_attr));
        FGPU_TRY(d_attr_vals.alloc(ctx, n_attr));
        FGPU_TRY(ctx->h2d(d_attr_ids.p, attr_ids, n_attr * sizeof(u64)));
        FGPU_TRY(ctx->h2d(d_attr_vals.p, attr_vals, n_attr * sizeof(double)));
        FGPU_TRY(launch(pw_attr_order_kernel, dim3(cdiv(n_attr, 256)), dim3(256), 0, st, (const u64*)d_attr_ids.p, (u32)n_attr, tot.p + 2));
    }
    if (!unit && n_attr == 0) FGPU_TRY(d_attr_ids.alloc(ctx, 1));   // (a list of nothing is still a list: every id takes `missing`)
    u32 h[11];
    if (n_ent == 0) {
        FGPU_TRY(read_words(ctx, tot.p, 3, h));
        FGPU_REQUIRE(h[2] == 0, FGPU_INVALID, "%s: attr_ids is not strictly ascending (%u adjacent pairs are not)", fn, h[2]);
        return finish_empty();
    }
    // ---- entries -----------------------------------------------------------------------------------------------------------
    std::vector<DevBuf<u32>> wr(L);
    std::vector<const u32*> hwr(L, nullptr);
    for (u32 l = 0; l < L; ++l) {
        const fgpu_mat* a = (l & 1u) ? vdp[l >> 1] : vm[l >> 1];
        if (!a || !a->nnz) continue;
        FGPU_TRY(wordrow_build(ctx, a->rowptr, a->nvec, a->nnz, wr[l]));
        hwr[l] = wr[l].p;
    }
    DevBuf<EeType> dty;
    DevBuf<u32> dlbase;
    DevBuf<const u32*> dlwr;
    DevBuf<u64> dactive;
    const u64 words = (n + 63) / 64;
    FGPU_TRY(dty.alloc(ctx, (size_t)T));
    FGPU_TRY(dlbase.alloc(ctx, (size_t)L + 1));
    FGPU_TRY(dlwr.alloc(ctx, L));
    if (active_bitmap) FGPU_TRY(dactive.alloc(ctx, words));
    FGPU_TRY(ctx->h2d(dty.p, hty.data(), (size_t)T * sizeof(EeType)));
    FGPU_TRY(ctx->h2d(dlbase.p, lbase.data(), ((size_t)L + 1) * sizeof(u32)));
    FGPU_TRY(ctx->h2d(dlwr.p, hwr.data(), (size_t)L * sizeof(const u32*)));
    if (active_bitmap) FGPU_TRY(ctx->h2d(dactive.p, active_bitmap, words * sizeof(u64)));
    PwIn in;
    in.ty = dty.p;
    in.lbase = dlbase.p;
    in.lwr = dlwr.p;
    in.active = active_bitmap ? dactive.p : nullptr;
    in.L = L;
    DevBuf<u32> ent_src, ent_dst, ent_ty, rel_off;
    DevBuf<u64> ent_val;
    FGPU_TRY(ent_src.alloc(ctx, n_ent));
    FGPU_TRY(ent_dst.alloc(ctx, n_ent));
    FGPU_TRY(ent_ty.alloc(ctx, n_ent));
    FGPU_TRY(ent_val.alloc(ctx, n_ent));
    FGPU_TRY(rel_off.alloc(ctx, (size_t)n_ent + 1));
    {
        ProfScope prof(ctx, "pw_entries", (u64)n_ent * 36);   // (plus the dp / dm probes of every m entry)
        FGPU_TRY(launch(pw_entry_kernel, dim3(cdiv((u64)n_ent + 1, 256)), dim3(256), 0, st, in, n_ent, ent_src.p, ent_dst.p, ent_val.p,
                        ent_ty.p, rel_off.p, (u64*)tot.p, tot.p + 3));
    }
    FGPU_TRY(read_words(ctx, tot.p, 6, h));
    FGPU_REQUIRE(h[2] == 0, FGPU_INVALID, "%s: attr_ids is not strictly ascending (%u adjacent pairs are not)", fn, h[2]);
    FGPU_REQUIRE(h[3] == 0, FGPU_INVALID, "%s: %u examined pairs hold MULTI_EDGE in a tensor, and its table has no row for them", fn, h[3]);
    const u64 n_rel64 = (u64)h[0] | ((u64)h[1] << 32);
    const u64 n_exam = h[4], n_multi = h[5];
    FGPU_REQUIRE(n_rel64 * (both ? 2u : 1u) < 0xFFFFFFFFull, FGPU_INVALID, "%s: %llu relationships give candidates past the 32-bit position space",
                 fn, (unsigned long long)n_rel64);
    const u32 n_rel = (u32)n_rel64;
    if (stats) {
        stats[0] = n_exam;
        stats[1] = n_rel;
        stats[6] = n_multi;
    }
    if (n_rel == 0) return finish_empty();
    // ---- weights -----------------------------------------------------------------------------------------------------------
    DevBuf<u32> wr_rel, rel_ent, rel_pos;
    DevBuf<u64> rel_key, rel_id;
    FGPU_TRY(scan_u32(ctx, rel_off.p, rel_off.p, (u64)n_ent + 1, nullptr));
    FGPU_TRY(wordrow_build(ctx, rel_off.p, n_ent, n_rel, wr_rel));
    FGPU_TRY(rel_ent.alloc(ctx, n_rel));
    FGPU_TRY(rel_pos.alloc(ctx, (size_t)n_rel + 1));
    FGPU_TRY(rel_key.alloc(ctx, n_rel));
    FGPU_TRY(rel_id.alloc(ctx, n_rel));
    PwAttr at;
    at.ids = unit ? nullptr : d_attr_ids.p;
    at.vals = d_attr_vals.p;
    at.n = (u32)n_attr;
    at.flags = flags;
    at.missing = missing;
    {
        ProfScope prof(ctx, "pw_weights", (u64)n_rel * 32);   // (plus one line per step of the attribute search)
        FGPU_TRY(launch(pw_rel_kernel, dim3(cdiv((u64)n_rel + 1, 256)), dim3(256), 0, st, in, at, (const u32*)rel_off.p, (const u32*)wr_rel.p,
                        n_rel, (const u64*)ent_val.p, (const u32*)ent_ty.p, rel_key.p, rel_id.p, rel_ent.p, rel_pos.p, d_refused.p,
                        tot.p + 6));
    }
    FGPU_TRY(scan_u32(ctx, rel_pos.p, rel_pos.p, (u64)n_rel + 1, tot.p + 8));
    u64 refused = ~0ull;
    FGPU_TRY(read_u64(ctx, d_refused.p, &refused));
    if (refused != ~0ull) {
        if (refused_id) *refused_id = refused;
        if (stats) memset(stats, 0, 8 * sizeof(u64));
        set_error("%s: relationship %llu has a negative weight", fn, (unsigned long long)refused);
        return FGPU_INVALID;
    }
    FGPU_TRY(read_words(ctx, tot.p + 6, 3, h));
    const u32 n_keep = h[2];
    const u64 n_cand = (u64)n_keep * (both ? 2u : 1u);
    if (stats) {
        stats[2] = n_cand;
        stats[4] = h[0];
        stats[5] = h[1];
    }
    if (n_cand == 0) return finish_empty();
    const dim3 cgrid(cdiv(n_cand, 256));
    // ---- candidates --------------------------------------------------------------------------------------------------------
    DevBuf<u32> c_from, c_to;
    DevBuf<u64> c_key, c_id;
    FGPU_TRY(c_from.alloc(ctx, n_cand));
    FGPU_TRY(c_to.alloc(ctx, n_cand));
    FGPU_TRY(c_key.alloc(ctx, n_cand));
    FGPU_TRY(c_id.alloc(ctx, n_cand));
    {
        ProfScope prof(ctx, "pw_place", (u64)n_rel * 24 + n_cand * 24);
        FGPU_TRY(launch(pw_place_kernel, dim3(cdiv(n_rel, 256)), dim3(256), 0, st, (const u32*)rel_pos.p, n_rel, flags, (const u32*)rel_ent.p,
                        (const u64*)rel_key.p, (const u64*)rel_id.p, (const u32*)ent_src.p, (const u32*)ent_dst.p, c_from.p, c_to.p, c_key.p,
                        c_id.p));
    }
    ent_src.release(); ent_dst.release(); ent_ty.release(); ent_val.release(); rel_off.release(); wr_rel.release();
    rel_ent.release(); rel_pos.release(); rel_key.release(); rel_id.release();
    // ---- group -------------------------------------------------------------------------------------------------------------
    DevBuf<u32> perm;
    FGPU_TRY(perm.alloc(ctx, n_cand));
    {
        ProfScope prof(ctx, "pw_sort", 0);
        DevBuf<u32> iota, keys, perm1;
        FGPU_TRY(iota.alloc(ctx, n_cand));
        FGPU_TRY(keys.alloc(ctx, n_cand));
        FGPU_TRY(perm1.alloc(ctx, n_cand));
        FGPU_TRY(launch(pw_iota_kernel, cgrid, dim3(256), 0, st, iota.p, n_cand));
        FGPU_TRY(pw_sort_pass(ctx, c_to.p, iota.p, n_cand, n, keys.p, perm1.p));
        FGPU_TRY(pw_sort_pass(ctx, c_from.p, perm1.p, n_cand, n, keys.p, perm.p));
    }
    // ---- reduce ------------------------------------------------------------------------------------------------------------
    DevBuf<u64> s_pair, s_key, s_id, min_key, min_id;
    DevBuf<u32> E, start;
    FGPU_TRY(s_pair.alloc(ctx, n_cand));
    FGPU_TRY(s_key.alloc(ctx, n_cand));
    FGPU_TRY(s_id.alloc(ctx, n_cand));
    FGPU_TRY(E.alloc(ctx, n_cand));
    u32 n_pairs = 0;
    {
        ProfScope prof(ctx, "pw_runs", n_cand * 56);
        FGPU_TRY(launch(pw_sorted_kernel, cgrid, dim3(256), 0, st, (const u32*)c_from.p, (const u32*)c_to.p, (const u64*)c_key.p,
                        (const u64*)c_id.p, (const u32*)perm.p, n_cand, s_pair.p, s_key.p, s_id.p));
        perm.release(); c_from.release(); c_to.release(); c_key.release(); c_id.release();
        FGPU_TRY(launch(pw_head_kernel, cgrid, dim3(256), 0, st, (const u64*)s_pair.p, n_cand, E.p));
        FGPU_TRY(scan_u32(ctx, E.p, E.p, n_cand, tot.p + 9));
        FGPU_TRY(read_u32(ctx, tot.p + 9, &n_pairs));
    }
    FGPU_REQUIRE(n_pairs >= 1 && n_pairs <= n_cand, FGPU_DEVICE, "%s: %u pairs of %llu candidates", fn, n_pairs, (unsigned long long)n_cand);
    const bool w_vals = W_out && !unit;
    MatRef first, second;   // the two outputs share one pattern: the second is a copy of the first's
    FGPU_TRY(mat_alloc(ctx, &first.m, n, n, n_pairs, W_out ? w_vals : true, 0, false));
    if (W_out && K_out) FGPU_TRY(mat_alloc(ctx, &second.m, n, n, n_pairs, true, 0, false));
    FGPU_TRY(min_key.alloc(ctx, n_pairs));
    FGPU_TRY(min_id.alloc(ctx, n_pairs));
    FGPU_TRY(start.alloc(ctx, (size_t)n_pairs + 1));
    FGPU_HIP(hipMemsetAsync(min_key.p, 0xFF, (size_t)n_pairs * sizeof(u64), st));
    FGPU_HIP(hipMemsetAsync(min_id.p, 0xFF, (size_t)n_pairs * sizeof(u64), st));
    {
        ProfScope prof(ctx, "pw_reduce", n_cand * 56 + (u64)n_pairs * 24);
        FGPU_TRY(launch(pw_min_key_kernel, cgrid, dim3(256), 0, st, (const u64*)s_pair.p, (const u64*)s_key.p, (const u64*)s_id.p,
                        (const u32*)E.p, n_cand, n_pairs, first->colidx, start.p, min_key.p, min_id.p));
        FGPU_TRY(launch(pw_min_id_kernel, cgrid, dim3(256), 0, st, (const u64*)s_pair.p, (const u64*)s_key.p, (const u64*)s_id.p,
                        (const u32*)E.p, n_cand, (const u64*)min_key.p, min_id.p));
    }
    {
        ProfScope prof(ctx, "pw_emit", (u64)n_pairs * 40 + n * 4);
        fgpu_mat* kmat = K_out ? (W_out ? second.get() : first.get()) : nullptr;
        FGPU_TRY(launch(pw_emit_kernel, dim3(cdiv(n_pairs, 256)), dim3(256), 0, st, (const u64*)min_key.p, (const u64*)min_id.p,
                        (const u32*)start.p, n_pairs, w_vals ? first->vals : (u64*)nullptr, kmat ? kmat->vals : (u64*)nullptr, tot.p + 10));
        FGPU_TRY(launch(pw_rowptr_kernel, dim3(cdiv(n + 1, 256)), dim3(256), 0, st, (const u64*)s_pair.p, n_cand, (const u32*)E.p, n_pairs,
                        n, first->rowptr));
        if (second.get()) {
            FGPU_HIP(hipMemcpyAsync(second->rowptr, first->rowptr, (n + 1) * sizeof(u32), hipMemcpyDeviceToDevice, st));
            FGPU_HIP(hipMemcpyAsync(second->colidx, first->colidx, (size_t)n_pairs * sizeof(u32), hipMemcpyDeviceToDevice, st));
        }
    }
    u32 longest = 0;
    FGPU_TRY(read_u32(ctx, tot.p + 10, &longest));
    FGPU_TRY(mat_finalize(first.get()));
    if (second.get()) FGPU_TRY(mat_finalize(second.get()));
    if (stats) {
        stats[3] = n_pairs;
        stats[7] = longest;
    }
    if (W_out) *W_out = first.release();
    if (K_out) *K_out = W_out ? second.release() : first.release();
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_pair_weights(fgpu_ctx* ctx, const fgpu_mat* const* m, const fgpu_mat* const* dp, const fgpu_mat* const* dm,
                                       const fgpu_multi* const* multi, int n_types, int flags, const uint64_t* active_bitmap,
                                       const uint64_t* attr_ids, const double* attr_vals, uint64_t n_attr, double missing,
                                       fgpu_mat** W, fgpu_mat** K, uint64_t* refused_id, uint64_t stats[8]) {
    return published(ctx, pair_weights_impl(ctx, m, dp, dm, multi, n_types, flags, active_bitmap, attr_ids, attr_vals, n_attr, missing,
                                            W, K, refused_id, stats));
}
