// expand_trails.hip — fgpu_expand_trails: CondVarLenTraverse (cond_var_len_traverse.rs:81-387, VarLenIter) for a whole batch of
// rows, without the attribute / WHERE filters.  The reference runs one LIFO DFS per row and builds every frame's adjacency with
// a matrix iterator; here the frames of all rows advance level by level, and the DFS order is computed afterwards with scans.
//
// A frame is (row, node, parent frame of the level before, edge id that led to it); level 0 holds the k roots.  The level step:
//   segments    a lane per (frame, type, half, layer): the stored run it walks — the node's row of m / dp for the outgoing half, of
//               mt_m / mt_dp for the incoming half — and its length.  S = exclusive scan of the lengths
//   gather      a lane per walked entry, its segment through the wordrow index over S (bulk.hpp): the pair's value as
//               ee_gather_kernel resolves it (dp shadow, dm tombstone, the forward value of an incoming entry), count = 1 or the
//               length of the table row under FGPU_MULTI_EDGE.  The item goes to its ADJACENCY slot: with one layer the entry
//               position; with a dp layer the position in the (frame, type, half) group after merging the two sorted runs —
//               own offset + the rank of the other node in the other run, a binary search, no sort
//   candidates  C = exclusive scan of the counts; a lane per candidate id: the used-edge test walks the parent links (at most
//               `depth` of them), then the emit and continue flags
//   place       exclusive scans of the two flags; child frames and emission records land in (parent, adjacency) order, so the
//               children and the emissions of a frame are contiguous: child_beg / emit_beg per frame
// The reference's order (frames leave a LIFO stack; a frame's emissions come before any deeper frame's) with E(F) = emitting
// children of F and S(F) = E(F) + sum of S over F's child frames:
//   sum         bottom-up per level, S(F) = E(F) + P[child_end] - P[child_beg] with P the exclusive scan of S over the level below
//   base        top-down per level, child c of F: base(c) = base(F) + E(F) + P[child_end(F)] - P[c + 1] (the later siblings run
//               first); base(root_i) = P_0[i] + the 0-hop rows up to and including row i
//   emit        a lane per emission: position base(parent) + its rank among the parent's emissions; under PATHS the path offsets
//               are one more scan (of the hops, in output order) and the lane walks its parent links to fill its path
// The only atomics are counters that place nothing.  No wavefront per frame: a hub node is as many lanes as it has entries.
#include "edge_layers.hpp"

namespace fgpu {

constexpr u32 ET_MAX_DEPTH = FGPU_TRAILS_MAX_DEPTH;

struct EtLv {   // the frames of one level
    const u32 *row, *node, *parent;
    const u64* edge;
};
struct EtBatch {
    const u32* dest;           // k, ~0u = unbound
    const EeType* ty;          // T
    const u64* bm;             // nullable
    const EtLv* lv;            // ET_MAX_DEPTH + 1 levels
    u32 T, H, L;               // types, halves walked (2: outgoing then incoming), layers (1: m only, 2: m and dp)
    u32 in_only;               // H == 1 and the half is the incoming one
    u32 min_hops, max_hops;
    u32 depth;                 // of the frames being expanded
    u32 reversed;
};
struct EtSeg { u32 f, t, l; bool in; };
__device__ __forceinline__ EtSeg et_seg(const EtBatch& b, u32 s) {
    EtSeg w;
    w.l = s % b.L; s /= b.L;
    const u32 h = s % b.H; s /= b.H;
    w.t = s % b.T;
    w.f = s / b.T;
    w.in = b.in_only || h == 1;
    return w;
}
__device__ __forceinline__ const CsrView& et_layer(const EeType& y, bool in, u32 l) {
    return in ? (l ? y.tdp : y.tm) : (l ? y.dp : y.m);
}

// seg_b[s] = first position of the run, seg_len[s] = its length (seg_len[nseg] = 0, so that the scan ends in the total)
__global__ __launch_bounds__(256) void et_segment_kernel(EtBatch b, u32 nseg, u32* __restrict__ seg_b, u32* __restrict__ seg_len,
                                                        u64* __restrict__ total) {
    const u64 s64 = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 len = 0;
    if (s64 < nseg) {
        const u32 s = (u32)s64;
        const EtSeg w = et_seg(b, s);
        u32 beg = 0, end = 0;
        row_range(et_layer(b.ty[w.t], w.in, w.l), b.lv[b.depth].node[w.f], beg, end);
        len = end - beg;
        seg_b[s] = beg;
        seg_len[s] = len;
    } else if (s64 == nseg) {
        seg_len[nseg] = 0u;
    }
    ee_add(len, total);
}

// cnt: [0] pairs that hold MULTI_EDGE without a table row [1] multi-edge pairs expanded.  The item of entry e lands at its
// adjacency slot p: it_frame / it_other (the neighbour) / it_val (the inline id, or the start of the table row when it_ty has
// bit 31 set; it_ty & 63 = the type position) / it_cnt (0: the entry holds no edge of the effective structure)
__global__ __launch_bounds__(256) void et_gather_kernel(EtBatch b, const u32* __restrict__ seg_b, const u32* __restrict__ seg_off,
                                                       const u32* __restrict__ wordrow, u32 n_ent, u32* __restrict__ it_frame,
                                                       u32* __restrict__ it_other, u64* __restrict__ it_val, u32* __restrict__ it_ty,
                                                       u32* __restrict__ it_cnt, u64* __restrict__ total, u32* __restrict__ cnt) {
    const u64 e64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool missing = false, multi = false;
    u32 c = 0;
    if (e64 < n_ent) {
        const u32 e = (u32)e64;
        const u32 s = entry_vec(seg_off, wordrow, e);
        const EtSeg w = et_seg(b, s);
        const EeType& y = b.ty[w.t];
        const u32 at = e - seg_off[s], q = seg_b[s] + at;
        const u32 node = b.lv[b.depth].node[w.f];
        const u32 other = et_layer(y, w.in, w.l).colidx[q];
        bool valid;
        u64 v = 0;
        if (!w.in) {
            if (w.l) {
                v = y.dpval[q];
                valid = true;
            } else {
                valid = probe(y.dp, node, other) == ~0u && probe(y.dm, node, other) == ~0u;   // (a shadowed pair is the dp item's)
                v = y.mval[q];
            }
        } else {
            const bool hidden = probe(y.tdm, node, other) != ~0u;
            valid = w.l ? (hidden || probe(y.tm, node, other) == ~0u) : !hidden;   // (a pair in both layers is the base item's)
            if (valid) valid = ee_value(y, other, node, v);
            if (b.H == 2 && other == node) valid = false;   // the outgoing half gave the self-loop
        }
        u32 tyw = w.t;
        if (valid) {
            c = 1;
            if (v == FGPU_MULTI_EDGE) {
                const u64 key = w.in ? (((u64)other << 32) | node) : (((u64)node << 32) | other);
                const u32 r = find(y.mkey, 0u, y.n_multi, key);
                if (r == ~0u) {
                    missing = true;
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
        // the slot: both runs of a (frame, type, half) group ascend by the other node; of one pair, m's entry goes first
        u32 p = e;
        if (b.L == 2) {
            const u32 so = s ^ 1u, ob = seg_b[so], oe = ob + (seg_off[so + 1] - seg_off[so]);
            const u32* __restrict__ ocol = et_layer(y, w.in, w.l ^ 1u).colidx;
            const u32 rank = lower_bound(ocol, ob, oe, w.l ? other + 1u : other) - ob;
            p = seg_off[s - w.l] + at + rank;
        }
        it_frame[p] = w.f;
        it_other[p] = other;
        it_val[p] = v;
        it_ty[p] = tyw;
        it_cnt[p] = c;
    } else if (e64 == n_ent) {
        it_cnt[n_ent] = 0u;
    }
    ee_add(c, total);
    count_if(missing, cnt + 0);
    count_if(multi, cnt + 1);
}

// cnt: [0] child frames [1] emissions [2] candidates dropped as already on the trail
__global__ __launch_bounds__(256) void et_cand_kernel(EtBatch b, const u32* __restrict__ cand_off, const u32* __restrict__ wordrow,
                                                     u32 n_cand, const u32* __restrict__ it_frame, const u32* __restrict__ it_other,
                                                     const u64* __restrict__ it_val, const u32* __restrict__ it_ty,
                                                     u32* __restrict__ c_item, u64* __restrict__ c_id, u32* __restrict__ c_cont,
                                                     u32* __restrict__ c_emit, u32* __restrict__ cnt) {
    const u64 c64 = (u64)blockIdx.x * 256 + threadIdx.x;
    bool used = false, emit = false, cont = false;
    if (c64 < n_cand) {
        const u32 c = (u32)c64;
        const u32 j = entry_vec(cand_off, wordrow, c);
        const u32 tyw = it_ty[j];
        const u64 v = it_val[j];
        const u64 id = (tyw & 0x80000000u) ? b.ty[tyw & 63u].mids[(u32)v + (c - cand_off[j])] : v;
        const u32 f0 = it_frame[j], nb = it_other[j];
        u32 f = f0;
        for (u32 l = b.depth; l >= 1; --l) {   // by id only, across types and directions (:247)
            const EtLv& lv = b.lv[l];
            if (lv.edge[f] == id) { used = true; break; }
            f = lv.parent[f];
        }
        if (!used) {
            const u32 hop = b.depth + 1, d = b.dest[b.lv[b.depth].row[f0]];
            emit = hop >= b.min_hops && (d == ~0u || d == nb) && (!b.bm || ee_bit(b.bm, nb));
            cont = hop < b.max_hops;
        }
        c_item[c] = j;
        c_id[c] = id;
        c_cont[c] = cont;
        c_emit[c] = emit;
    } else if (c64 == n_cand) {
        c_cont[n_cand] = 0u;
        c_emit[n_cand] = 0u;
    }
    count_if(cont, cnt + 0);
    count_if(emit, cnt + 1);
    count_if(used, cnt + 2);
}

// cont_off / emit_off: the exclusive scans of the flags (n_cand + 1 each)
__global__ __launch_bounds__(256) void et_place_kernel(EtBatch b, u32 n_cand, const u32* __restrict__ c_item, const u64* __restrict__ c_id,
                                                      const u32* __restrict__ cont_off, const u32* __restrict__ emit_off,
                                                      const u32* __restrict__ it_frame, const u32* __restrict__ it_other,
                                                      u32* __restrict__ nx_row, u32* __restrict__ nx_node, u32* __restrict__ nx_parent,
                                                      u64* __restrict__ nx_edge, u32* __restrict__ em_parent, u32* __restrict__ em_node,
                                                      u64* __restrict__ em_edge) {
    const u64 c64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (c64 >= n_cand) return;
    const u32 c = (u32)c64, j = c_item[c], f = it_frame[j], nb = it_other[j];
    const u32 x = cont_off[c], o = emit_off[c];
    if (cont_off[c + 1] != x) {
        nx_row[x] = b.lv[b.depth].row[f];
        nx_node[x] = nb;
        nx_parent[x] = f;
        nx_edge[x] = c_id[c];
    }
    if (emit_off[c + 1] != o) {
        em_parent[o] = f;
        em_node[o] = nb;
        em_edge[o] = c_id[c];
    }
}

// child_beg[f] / emit_beg[f] (f <= nf): the first child frame / emission of frame f, through its first entry and candidate
__global__ __launch_bounds__(256) void et_frame_kernel(u32 nf, u32 per_frame, const u32* __restrict__ seg_off, const u32* __restrict__ cand_off,
                                                      const u32* __restrict__ cont_off, const u32* __restrict__ emit_off,
                                                      u32* __restrict__ child_beg, u32* __restrict__ emit_beg) {
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f > nf) return;
    const u32 c0 = cand_off[seg_off[(u32)f * per_frame]];
    child_beg[f] = cont_off[c0];
    emit_beg[f] = emit_off[c0];
}

// S[f] = E(f) + the S of f's children (P_below: the exclusive scan of S over the level below, nullable); S[nf] = 0
__global__ __launch_bounds__(256) void et_sum_kernel(u32 nf, const u32* __restrict__ child_beg, const u32* __restrict__ emit_beg,
                                                    const u32* __restrict__ P_below, u32* __restrict__ S) {
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f > nf) return;
    u32 s = 0;
    if (f < nf) {
        s = emit_beg[f + 1] - emit_beg[f];
        if (P_below) s += P_below[child_beg[f + 1]] - P_below[child_beg[f]];
    }
    S[f] = s;
}

// base of the roots: zx = the 0-hop rows before row i (k + 1 entries); the 0-hop row itself is written here
__global__ __launch_bounds__(256) void et_root_kernel(u32 k, u32 reversed, const u32* __restrict__ P, const u32* __restrict__ zx,
                                                     const u32* __restrict__ start, u32* __restrict__ base, u32* __restrict__ o_row,
                                                     u32* __restrict__ o_from, u32* __restrict__ o_to, u32* __restrict__ o_hops) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const u32 o = P[i] + zx[i], z = zx[i + 1] - zx[i];
    base[i] = o + z;
    if (z) {
        o_row[o] = (u32)i;
        o_from[o] = o_to[o] = start[i];
        o_hops[o] = 0u;
    }
}
// base of level d + 1 from level d: the later siblings' subtrees come first
__global__ __launch_bounds__(256) void et_base_kernel(u32 n_child, const u32* __restrict__ parent, const u32* __restrict__ base_up,
                                                     const u32* __restrict__ child_beg_up, const u32* __restrict__ emit_beg_up,
                                                     const u32* __restrict__ P, u32* __restrict__ base) {
    const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_child) return;
    const u32 p = parent[c];
    base[c] = base_up[p] + (emit_beg_up[p + 1] - emit_beg_up[p]) + (P[child_beg_up[p + 1]] - P[c + 1]);
}

// the emissions of the frames of level b.depth
__global__ __launch_bounds__(256) void et_emit_kernel(EtBatch b, u32 n_emit, u32 n_out, const u32* __restrict__ em_parent, const u32* __restrict__ em_node,
                                                     const u32* __restrict__ emit_beg, const u32* __restrict__ base,
                                                     u32* __restrict__ o_row, u32* __restrict__ o_from, u32* __restrict__ o_to,
                                                     u32* __restrict__ o_hops) {
    const u64 j64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j64 >= n_emit) return;
    const u32 j = (u32)j64, p = em_parent[j], o = base[p] + (j - emit_beg[p]);
    if (o >= n_out) return;   // (never: the bases partition the output)
    const u32 row = b.lv[b.depth].row[p], s = b.lv[0].node[row], nb = em_node[j];
    o_row[o] = row;
    o_from[o] = b.reversed ? nb : s;
    o_to[o] = b.reversed ? s : nb;
    o_hops[o] = b.depth + 1;
}
// ... and their paths: h edges at path_off[o], h + 1 nodes at path_off[o] + o, in pattern order (reversed under REVERSED)
__global__ __launch_bounds__(256) void et_path_kernel(EtBatch b, u32 n_emit, u32 n_out, const u32* __restrict__ em_parent, const u32* __restrict__ em_node,
                                                     const u64* __restrict__ em_edge, const u32* __restrict__ emit_beg,
                                                     const u32* __restrict__ base, const u64* __restrict__ path_off,
                                                     u32* __restrict__ p_node, u64* __restrict__ p_edge) {
    const u64 j64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j64 >= n_emit) return;
    const u32 j = (u32)j64, p = em_parent[j], o = base[p] + (j - emit_beg[p]);
    if (o >= n_out) return;
    const u32 h = b.depth + 1;
    u64* __restrict__ pe = p_edge + path_off[o];
    u32* __restrict__ pn = p_node + path_off[o] + o;
    // step i (1 .. h) = (edge i, node i); node 0 is the start
    pe[b.reversed ? 0u : h - 1] = em_edge[j];
    pn[b.reversed ? 0u : h] = em_node[j];
    u32 f = p;
    for (u32 l = b.depth; l >= 1; --l) {
        const EtLv& lv = b.lv[l];
        pe[b.reversed ? h - l : l - 1] = lv.edge[f];
        pn[b.reversed ? h - l : l] = lv.node[f];
        f = lv.parent[f];
    }
    pn[b.reversed ? h : 0u] = b.lv[0].node[f];
}
// the one node of a 0-hop row
__global__ __launch_bounds__(256) void et_path0_kernel(u32 k, const u32* __restrict__ P, const u32* __restrict__ zx, const u32* __restrict__ start,
                                                      const u64* __restrict__ path_off, u32* __restrict__ p_node) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= k || zx[i + 1] == zx[i]) return;
    const u32 o = P[i] + zx[i];
    p_node[path_off[o] + o] = start[i];
}

struct EtLevel {   // what a level keeps until the order is known
    u32 nf = 0, n_emit = 0;
    DevBuf<u32> row, node, parent, child_beg, emit_beg, em_parent, em_node, P, base;
    DevBuf<u64> edge, em_edge;
};

static fgpu_info expand_trails_impl(fgpu_ctx* ctx, const u64* start, const u64* dest, u64 k, const fgpu_mat* const* m,
                                    const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                                    const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                                    int n_types, int flags, u32 min_hops, u32 max_hops, const u64* bitmap, u64 max_items, u32** out_row,
                                    u32** out_from, u32** out_to, u32** out_hops, u64** out_path_off, u32** out_path_node,
                                    u64** out_path_edge, u64* out_n, u64* st) {
    const char* fn = "fgpu_expand_trails";
    FGPU_REQUIRE(ctx && out_row && out_from && out_to && out_hops && out_n, FGPU_NULL_POINTER, "%s: NULL argument", fn);
    *out_row = *out_from = *out_to = *out_hops = nullptr;
    *out_n = 0;
    if (out_path_off) *out_path_off = nullptr;
    if (out_path_node) *out_path_node = nullptr;
    if (out_path_edge) *out_path_edge = nullptr;
    FGPU_REQUIRE((flags & ~7) == 0, FGPU_INVALID, "%s: unknown flag bits in %d", fn, flags);
    const bool reversed = flags & FGPU_TRAILS_REVERSED, bidir = flags & FGPU_TRAILS_BIDIRECTIONAL, paths = flags & FGPU_TRAILS_PATHS;
    FGPU_REQUIRE(!(reversed && bidir), FGPU_INVALID, "%s: REVERSED and BIDIRECTIONAL exclude each other", fn);
    FGPU_REQUIRE(paths ? (out_path_off && out_path_node && out_path_edge) : (!out_path_off && !out_path_node && !out_path_edge),
                 paths ? FGPU_NULL_POINTER : FGPU_INVALID, "%s: the three path outputs go with FGPU_TRAILS_PATHS, and only with it", fn);
    FGPU_REQUIRE(k == 0 || start, FGPU_NULL_POINTER, "%s: NULL start", fn);
    FGPU_REQUIRE(n_types == 0 || m, FGPU_NULL_POINTER, "%s: NULL m", fn);
    FGPU_REQUIRE(k <= EE_MAX_ROWS, FGPU_INVALID, "%s: %llu rows in one batch (at most %llu)", fn, (unsigned long long)k,
                 (unsigned long long)EE_MAX_ROWS);
    FGPU_REQUIRE(n_types >= 0 && n_types <= EE_MAX_TYPES, FGPU_INVALID, "%s: %d types (at most %d)", fn, n_types, EE_MAX_TYPES);
    FGPU_REQUIRE(max_items != 0 && max_items < 0xFFFFFFFFull, FGPU_INVALID, "%s: max_items = %llu is not in 1 .. 2^32 - 2", fn,
                 (unsigned long long)max_items);
    if (k == 0) return FGPU_OK;
    // ---- the layers ------------------------------------------------------------------------------------------------------
    u64 n = ~0ull;   // (no type: nothing bounds the ids, and nothing is walked)
    bool any_dp = false;
    std::vector<EeType> hty;
    const bool walk_in = reversed || bidir;
    if (n_types) {
        FGPU_TRY(ee_types(fn, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, hty, n, any_dp));
        if (walk_in)
            for (int t = 0; t < n_types; ++t)
                FGPU_REQUIRE(ee_at(mt_m, t), FGPU_INVALID, "%s: incoming entries are walked and mt_m[%d] is missing", fn, t);
    }
    // ---- the rows --------------------------------------------------------------------------------------------------------
    std::vector<u32> s32(k), d32(k), zx(k + 1, 0u);
    for (u64 i = 0; i < k; ++i) {
        const bool db = dest && dest[i] != ~0ull;
        FGPU_REQUIRE(start[i] < n && start[i] < 0xFFFFFFFFull && (!db || (dest[i] < n && dest[i] < 0xFFFFFFFFull)), FGPU_INVALID,
                     "%s: row %llu = (%llu, %llu) names a node at or past %llu", fn, (unsigned long long)i, (unsigned long long)start[i],
                     (unsigned long long)(dest ? dest[i] : ~0ull), (unsigned long long)n);
        s32[i] = (u32)start[i];
        d32[i] = db ? (u32)dest[i] : ~0u;
        // the 0-hop row (:153-171)
        const bool zero = min_hops == 0 && (!db || dest[i] == start[i]) && (!bitmap || ((bitmap[start[i] >> 6] >> (start[i] & 63)) & 1ull));
        zx[i + 1] = zx[i] + (zero ? 1u : 0u);
    }
    const u32 n_zero = zx[k];
    u64 held = k + n_zero;   // frames and emissions
    st[7] = held;
    st[3] = n_zero;
    FGPU_REQUIRE(held <= max_items, FGPU_INSUFFICIENT_SPACE, "%s: %llu rows and %u 0-hop rows exceed max_items = %llu", fn,
                 (unsigned long long)k, n_zero, (unsigned long long)max_items);
    hipStream_t stream = ctx->stream();
    EtBatch b;
    b.T = (u32)n_types;
    b.H = (bidir ? 2u : 1u);
    b.L = any_dp ? 2u : 1u;
    b.in_only = reversed;
    b.min_hops = min_hops;
    b.max_hops = max_hops;
    b.reversed = reversed;
    b.depth = 0;
    const u32 per_frame = b.T * b.H * b.L;
    st[5] = any_dp ? 1 : 0;
    // ---- level 0 and what every level reads ------------------------------------------------------------------------------------
    std::vector<EtLevel> lvl;
    lvl.reserve(ET_MAX_DEPTH + 2);   // (no level moves once the loop holds references)
    std::vector<EtLv> htab(ET_MAX_DEPTH + 1, EtLv{nullptr, nullptr, nullptr, nullptr});
    DevBuf<u32> ddest, dzx, tot;
    DevBuf<EeType> dty;
    DevBuf<EtLv> dtab;
    DevBuf<u64> dbm;
    const u64 words = n_types ? (n + 63) / 64 : 0;
    lvl.emplace_back();
    {
        EtLevel& r = lvl[0];
        r.nf = (u32)k;
        FGPU_TRY(r.row.alloc(ctx, k));
        FGPU_TRY(r.node.alloc(ctx, k));
        FGPU_TRY(ddest.alloc(ctx, k));
        FGPU_TRY(dzx.alloc(ctx, k + 1));
        FGPU_TRY(dty.alloc(ctx, (size_t)n_types));
        FGPU_TRY(dtab.alloc(ctx, ET_MAX_DEPTH + 1));
        FGPU_TRY(tot.alloc(ctx, 16));
        if (bitmap && words) FGPU_TRY(dbm.alloc(ctx, words));
        std::vector<u32> iota(k);
        for (u64 i = 0; i < k; ++i) iota[i] = (u32)i;
        ProfScope up(ctx, "et_h2d", k * 16 + (size_t)n_types * sizeof(EeType) + words * 8);
        FGPU_TRY(ctx->h2d(r.row.p, iota.data(), k * sizeof(u32)));
        FGPU_TRY(ctx->h2d(r.node.p, s32.data(), k * sizeof(u32)));
        FGPU_TRY(ctx->h2d(ddest.p, d32.data(), k * sizeof(u32)));
        FGPU_TRY(ctx->h2d(dzx.p, zx.data(), (k + 1) * sizeof(u32)));
        if (n_types) FGPU_TRY(ctx->h2d(dty.p, hty.data(), (size_t)n_types * sizeof(EeType)));
        if (dbm.p) FGPU_TRY(ctx->h2d(dbm.p, bitmap, words * sizeof(u64)));
        htab[0] = EtLv{r.row.p, r.node.p, nullptr, nullptr};
    }
    b.dest = ddest.p;
    b.ty = dty.p;
    b.bm = dbm.p;
    b.lv = dtab.p;
    // ---- the levels ------------------------------------------------------------------------------------------------------------
    const bool run = n_types && max_hops >= 1 && min_hops <= max_hops;
    for (u32 d = 0; run && lvl[d].nf; ++d) {
        EtLevel& cur = lvl[d];
        const u32 nf = cur.nf;
        b.depth = d;
        st[0] += nf;
        st[4] = d + 1;
        FGPU_TRY(cur.child_beg.alloc(ctx, (size_t)nf + 1));
        FGPU_TRY(cur.emit_beg.alloc(ctx, (size_t)nf + 1));
        FGPU_HIP(hipMemsetAsync(cur.child_beg.p, 0, ((size_t)nf + 1) * sizeof(u32), stream));
        FGPU_HIP(hipMemsetAsync(cur.emit_beg.p, 0, ((size_t)nf + 1) * sizeof(u32), stream));
        FGPU_HIP(hipMemsetAsync(tot.p, 0, 16 * sizeof(u32), stream));
        FGPU_TRY(ctx->h2d(dtab.p, htab.data(), htab.size() * sizeof(EtLv)));
        const u64 nseg64 = (u64)nf * per_frame;
        FGPU_REQUIRE(nseg64 < (1ull << 31), FGPU_INSUFFICIENT_SPACE, "%s: %u frames x %u segments at depth %u exceed 2^31", fn, nf, per_frame, d);
        const u32 nseg = (u32)nseg64;
        // tot: [0..1] entries walked, [2..3] candidate ids (64-bit sums), [4..5] et_gather_kernel's cnt, [6..8] et_cand_kernel's
        DevBuf<u32> seg_b, seg_off, wr_seg;
        FGPU_TRY(seg_b.alloc(ctx, nseg));
        FGPU_TRY(seg_off.alloc(ctx, (size_t)nseg + 1));
        {
            ProfScope prof(ctx, "et_segments", (u64)nseg * 8);
            FGPU_TRY(launch(et_segment_kernel, dim3(cdiv((u64)nseg + 1, 256)), dim3(256), 0, stream, b, nseg, seg_b.p, seg_off.p, (u64*)tot.p));
        }
        u32 h[9];
        FGPU_TRY(read_words(ctx, tot.p, 2, h));
        const u64 n_ent64 = (u64)h[0] | ((u64)h[1] << 32);
        FGPU_REQUIRE(n_ent64 < 0xFFFFFFFFull, FGPU_INSUFFICIENT_SPACE, "%s: depth %u walks %llu stored entries, past the 32-bit position space",
                     fn, d, (unsigned long long)n_ent64);
        const u32 n_ent = (u32)n_ent64;
        st[1] += n_ent;
        if (n_ent == 0) break;
        FGPU_TRY(scan_u32(ctx, seg_off.p, seg_off.p, (u64)nseg + 1, nullptr));
        FGPU_TRY(wordrow_build(ctx, seg_off.p, nseg, n_ent, wr_seg));
        DevBuf<u32> it_frame, it_other, it_ty, cand_off, wr_cand;
        DevBuf<u64> it_val;
        FGPU_TRY(it_frame.alloc(ctx, n_ent));
        FGPU_TRY(it_other.alloc(ctx, n_ent));
        FGPU_TRY(it_ty.alloc(ctx, n_ent));
        FGPU_TRY(cand_off.alloc(ctx, (size_t)n_ent + 1));
        FGPU_TRY(it_val.alloc(ctx, n_ent));
        {
            ProfScope prof(ctx, "et_gather", (u64)n_ent * 28);   // (plus one 64-byte line per probe step: the searches are the cost)
            FGPU_TRY(launch(et_gather_kernel, dim3(cdiv((u64)n_ent + 1, 256)), dim3(256), 0, stream, b, (const u32*)seg_b.p,
                            (const u32*)seg_off.p, (const u32*)wr_seg.p, n_ent, it_frame.p, it_other.p, it_val.p, it_ty.p, cand_off.p,
                            (u64*)(tot.p + 2), tot.p + 4));
        }
        FGPU_TRY(read_words(ctx, tot.p + 2, 4, h));
        FGPU_REQUIRE(h[2] == 0, FGPU_INVALID, "%s: %u walked pairs hold MULTI_EDGE in a tensor, and its table has no row for them", fn, h[2]);
        const u64 n_cand64 = (u64)h[0] | ((u64)h[1] << 32);
        FGPU_REQUIRE(n_cand64 < 0xFFFFFFFFull, FGPU_INSUFFICIENT_SPACE, "%s: depth %u walks %llu edge ids, past the 32-bit position space", fn, d,
                     (unsigned long long)n_cand64);
        const u32 n_cand = (u32)n_cand64;
        st[6] += h[3];
        if (n_cand == 0) break;
        FGPU_TRY(scan_u32(ctx, cand_off.p, cand_off.p, (u64)n_ent + 1, nullptr));
        FGPU_TRY(wordrow_build(ctx, cand_off.p, n_ent, n_cand, wr_cand));
        DevBuf<u32> c_item, cont_off, emit_off;
        DevBuf<u64> c_id;
        FGPU_TRY(c_item.alloc(ctx, n_cand));
        FGPU_TRY(c_id.alloc(ctx, n_cand));
        FGPU_TRY(cont_off.alloc(ctx, (size_t)n_cand + 1));
        FGPU_TRY(emit_off.alloc(ctx, (size_t)n_cand + 1));
        {
            ProfScope prof(ctx, "et_candidates", (u64)n_cand * 40);
            FGPU_TRY(launch(et_cand_kernel, dim3(cdiv((u64)n_cand + 1, 256)), dim3(256), 0, stream, b, (const u32*)cand_off.p,
                            (const u32*)wr_cand.p, n_cand, (const u32*)it_frame.p, (const u32*)it_other.p, (const u64*)it_val.p,
                            (const u32*)it_ty.p, c_item.p, c_id.p, cont_off.p, emit_off.p, tot.p + 6));
        }
        // the level's counts come back before its buffers are allocated
        FGPU_TRY(read_words(ctx, tot.p + 6, 3, h));
        const u32 n_cont = h[0], n_emit = h[1];
        st[2] += h[2];
        st[3] += n_emit;
        held += (u64)n_cont + n_emit;
        st[7] = held;
        FGPU_REQUIRE(held <= max_items, FGPU_INSUFFICIENT_SPACE, "%s: %llu frames and emissions after depth %u exceed max_items = %llu", fn,
                     (unsigned long long)held, d, (unsigned long long)max_items);
        FGPU_REQUIRE(n_cont == 0 || d < ET_MAX_DEPTH, FGPU_INSUFFICIENT_SPACE, "%s: %u trails go on past %u edges", fn, n_cont,
                     ET_MAX_DEPTH);
        cur.n_emit = n_emit;
        FGPU_TRY(scan_u32(ctx, cont_off.p, cont_off.p, (u64)n_cand + 1, nullptr));
        FGPU_TRY(scan_u32(ctx, emit_off.p, emit_off.p, (u64)n_cand + 1, nullptr));
        lvl.emplace_back();
        EtLevel& nx = lvl[d + 1];
        EtLevel& me = lvl[d];   // (lvl was reserved: cur stays valid; named again for the reader)
        nx.nf = n_cont;
        FGPU_TRY(nx.row.alloc(ctx, n_cont));
        FGPU_TRY(nx.node.alloc(ctx, n_cont));
        FGPU_TRY(nx.parent.alloc(ctx, n_cont));
        FGPU_TRY(nx.edge.alloc(ctx, n_cont));
        FGPU_TRY(me.em_parent.alloc(ctx, n_emit));
        FGPU_TRY(me.em_node.alloc(ctx, n_emit));
        FGPU_TRY(me.em_edge.alloc(ctx, n_emit));
        {
            ProfScope prof(ctx, "et_place", (u64)n_cand * 24 + ((u64)n_cont + n_emit) * 20);
            FGPU_TRY(launch(et_place_kernel, dim3(cdiv(n_cand, 256)), dim3(256), 0, stream, b, n_cand, (const u32*)c_item.p, (const u64*)c_id.p,
                            (const u32*)cont_off.p, (const u32*)emit_off.p, (const u32*)it_frame.p, (const u32*)it_other.p, nx.row.p,
                            nx.node.p, nx.parent.p, nx.edge.p, me.em_parent.p, me.em_node.p, me.em_edge.p));
            FGPU_TRY(launch(et_frame_kernel, dim3(cdiv((u64)nf + 1, 256)), dim3(256), 0, stream, nf, per_frame, (const u32*)seg_off.p,
                            (const u32*)cand_off.p, (const u32*)cont_off.p, (const u32*)emit_off.p, me.child_beg.p, me.emit_beg.p));
        }
        if (n_cont) htab[d + 1] = EtLv{nx.row.p, nx.node.p, nx.parent.p, nx.edge.p};
    }
    const u64 n_out64 = st[3];
    if (n_out64 == 0) return FGPU_OK;
    const u32 n_out = (u32)n_out64;   // (below max_items)
    u32 D = 0;                        // the expanded levels: every level but a last one without frames
    while (D < lvl.size() && lvl[D].child_beg.p) ++D;
    const bool levels = D != 0;
    FGPU_TRY(ctx->h2d(dtab.p, htab.data(), htab.size() * sizeof(EtLv)));
    // ---- the order ---------------------------------------------------------------------------------------------------------------
    {
        ProfScope prof(ctx, "et_order", held * 16);
        for (u32 d = D; d-- > 0;) {
            EtLevel& L = lvl[d];
            FGPU_TRY(L.P.alloc(ctx, (size_t)L.nf + 1));
            FGPU_TRY(launch(et_sum_kernel, dim3(cdiv((u64)L.nf + 1, 256)), dim3(256), 0, stream, L.nf, (const u32*)L.child_beg.p,
                            (const u32*)L.emit_beg.p, d + 1 < D ? (const u32*)lvl[d + 1].P.p : (const u32*)nullptr, L.P.p));
            FGPU_TRY(scan_u32(ctx, L.P.p, L.P.p, (u64)L.nf + 1, nullptr));
        }
        if (!levels) {   // only 0-hop rows
            FGPU_TRY(lvl[0].P.alloc(ctx, k + 1));
            FGPU_HIP(hipMemsetAsync(lvl[0].P.p, 0, (k + 1) * sizeof(u32), stream));
        }
    }
    DevBuf<u32> o_row, o_from, o_to, o_hops, p_node;
    DevBuf<u64> p_off, p_edge;
    FGPU_TRY(o_row.alloc(ctx, n_out));
    FGPU_TRY(o_from.alloc(ctx, n_out));
    FGPU_TRY(o_to.alloc(ctx, n_out));
    FGPU_TRY(o_hops.alloc(ctx, (size_t)n_out + 1));
    {
        ProfScope prof(ctx, "et_emit", (u64)n_out * 36);
        FGPU_TRY(lvl[0].base.alloc(ctx, k));
        FGPU_TRY(launch(et_root_kernel, dim3(cdiv(k, 256)), dim3(256), 0, stream, (u32)k, (u32)reversed, (const u32*)lvl[0].P.p,
                        (const u32*)dzx.p, (const u32*)lvl[0].node.p, lvl[0].base.p, o_row.p, o_from.p, o_to.p, o_hops.p));
        for (u32 d = 0; d < D; ++d) {
            EtLevel& L = lvl[d];
            if (d) {
                EtLevel& up = lvl[d - 1];
                FGPU_TRY(L.base.alloc(ctx, L.nf));
                FGPU_TRY(launch(et_base_kernel, dim3(cdiv(L.nf, 256)), dim3(256), 0, stream, L.nf, (const u32*)L.parent.p, (const u32*)up.base.p,
                                (const u32*)up.child_beg.p, (const u32*)up.emit_beg.p, (const u32*)L.P.p, L.base.p));
            }
            if (!L.n_emit) continue;
            b.depth = d;
            FGPU_TRY(launch(et_emit_kernel, dim3(cdiv(L.n_emit, 256)), dim3(256), 0, stream, b, L.n_emit, n_out, (const u32*)L.em_parent.p,
                            (const u32*)L.em_node.p, (const u32*)L.emit_beg.p, (const u32*)L.base.p, o_row.p, o_from.p, o_to.p, o_hops.p));
        }
    }
    u64 n_path = 0;
    if (paths) {
        ProfScope prof(ctx, "et_paths", (u64)n_out * 24);
        FGPU_TRY(p_off.alloc(ctx, (size_t)n_out + 1));
        FGPU_HIP(hipMemsetAsync(o_hops.p + n_out, 0, sizeof(u32), stream));
        FGPU_TRY(scan_u32_to_u64(ctx, o_hops.p, p_off.p, (u64)n_out + 1, nullptr));
        FGPU_TRY(read_u64(ctx, p_off.p + n_out, &n_path));
        FGPU_TRY(p_edge.alloc(ctx, n_path));
        FGPU_TRY(p_node.alloc(ctx, n_path + n_out));
        FGPU_TRY(launch(et_path0_kernel, dim3(cdiv(k, 256)), dim3(256), 0, stream, (u32)k, (const u32*)lvl[0].P.p, (const u32*)dzx.p,
                        (const u32*)lvl[0].node.p, (const u64*)p_off.p, p_node.p));
        for (u32 d = 0; d < D; ++d) {
            EtLevel& L = lvl[d];
            if (!L.n_emit) continue;
            b.depth = d;
            FGPU_TRY(launch(et_path_kernel, dim3(cdiv(L.n_emit, 256)), dim3(256), 0, stream, b, L.n_emit, n_out, (const u32*)L.em_parent.p,
                            (const u32*)L.em_node.p, (const u64*)L.em_edge.p, (const u32*)L.emit_beg.p, (const u32*)L.base.p,
                            (const u64*)p_off.p, p_node.p, p_edge.p));
        }
    }
    // ---- out -----------------------------------------------------------------------------------------------------------------------
    ResultBuf rr, rf, rt, rh, ro, rn, re;
    FGPU_REQUIRE(rr.alloc(ctx, (size_t)n_out * 4) && rf.alloc(ctx, (size_t)n_out * 4) && rt.alloc(ctx, (size_t)n_out * 4) &&
                     rh.alloc(ctx, (size_t)n_out * 4) &&
                     (!paths || (ro.alloc(ctx, ((size_t)n_out + 1) * 8) && rn.alloc(ctx, (size_t)(n_path + n_out) * 4) &&
                                 re.alloc(ctx, (size_t)(n_path ? n_path : 1) * 8))),
                 FGPU_OOM, "%s: out of host memory", fn);
    {
        ProfScope prof(ctx, "et_readback", (u64)n_out * 16 + (paths ? (u64)n_out * 12 + n_path * 12 : 0));
        FGPU_TRY(ctx->d2h(rr.p, o_row.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(rf.p, o_from.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(rt.p, o_to.p, (size_t)n_out * 4));
        FGPU_TRY(ctx->d2h(rh.p, o_hops.p, (size_t)n_out * 4));
        if (paths) {
            FGPU_TRY(ctx->d2h(ro.p, p_off.p, ((size_t)n_out + 1) * 8));
            FGPU_TRY(ctx->d2h(rn.p, p_node.p, (size_t)(n_path + n_out) * 4));
            if (n_path) FGPU_TRY(ctx->d2h(re.p, p_edge.p, (size_t)n_path * 8));
        }
    }
    *out_row = (u32*)rr.release();
    *out_from = (u32*)rf.release();
    *out_to = (u32*)rt.release();
    *out_hops = (u32*)rh.release();
    if (paths) {
        *out_path_off = (u64*)ro.release();
        *out_path_node = (u32*)rn.release();
        *out_path_edge = (u64*)re.release();
    }
    *out_n = n_out;
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_expand_trails(fgpu_ctx* ctx, const uint64_t* start, const uint64_t* dest, uint64_t k, const fgpu_mat* const* m,
                                        const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                                        const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                                        int n_types, int flags, uint32_t min_hops, uint32_t max_hops, const uint64_t* dst_label_bitmap,
                                        uint64_t max_items, uint32_t** out_row, uint32_t** out_from, uint32_t** out_to,
                                        uint32_t** out_hops, uint64_t** out_path_off, uint32_t** out_path_node,
                                        uint64_t** out_path_edge, uint64_t* out_n, uint64_t stats[8]) {
    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const fgpu_info info = expand_trails_impl(ctx, start, dest, k, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, flags, min_hops, max_hops,
                                              dst_label_bitmap, max_items, out_row, out_from, out_to, out_hops, out_path_off,
                                              out_path_node, out_path_edge, out_n, st);
    if (stats) memcpy(stats, st, sizeof(st));
    return info;
}
