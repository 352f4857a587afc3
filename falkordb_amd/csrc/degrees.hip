// degrees.hip — fgpu_node_degrees: indegree(n [, types]) / outdegree(n [, types]) (entity.rs:268-381, graph.rs:1839-1887) for a
// batch of nodes or for every node.  The reference counts Tensor::iter(id, id, transposed) per node and type, one versioned
// row iterator each and every id of a multi-edge list walked; here a call is the count fgpu_expand_edges would emit per row,
// without its columns, sort and placement:
//
//   tiers     per (type, direction), decided on the host: the walked side has no dp, no dm and no table — the effective row IS
//             the stored row and every pair weighs 1 — or not
//   segments  a lane per (position, direction, type, layer).  Row-pointer tier: the layer-0 lane adds the stored row's length
//             to the position's counter and no entry is ever read.  Entry tier: the run the lane's layer (m / dp, or mt_m /
//             mt_dp) holds for the node and its length, as ee_segment_kernel.  S = exclusive scan of the lengths
//   count     a lane per walked entry, its segment recovered through the wordrow index over S (bulk.hpp): the dp shadow and the
//             dm tombstone by binary search, for an incoming entry the forward value at (src, node), exactly the tests of
//             ee_gather_kernel; weight 1, or the length of the table row under FGPU_MULTI_EDGE.  The entries of one (position,
//             direction) are consecutive, so the 64 weights of a wavefront are summed by run with shuffles and each run's head
//             lane adds once: one 64-bit atomicAdd per (wavefront, position, direction), none per entry
//
// Positions are walked in windows (degree_window_rows) so that one window's segments stay below 2^31 and its entries below
// 2^32 - 1; a window's counters are k words per direction and go to the caller through the lane's staging halves.
#include "edge_layers.hpp"

namespace fgpu {

struct DgBatch {
    const u32* nodes;          // nullable: position i is node base + i
    const EeType* ty;          // T
    u64 fast[2];               // bit t: (type t, outgoing / incoming) is answered from the row pointers
    u32 base, rows, D, T, L;   // positions of the window, directions, types, layers (1: base only, 2: base and dp)
    u32 dir0;                  // the direction when D == 1: 0 outgoing, 1 incoming (D == 2: index 0 outgoing, 1 incoming)
};
struct DgWalk { u32 i, d, t, l, in, v; };
__device__ __forceinline__ DgWalk dg_walk(const DgBatch& b, u32 s) {
    DgWalk w;
    w.l = s % b.L; s /= b.L;
    w.t = s % b.T; s /= b.T;
    w.d = s % b.D;
    w.i = s / b.D;
    w.in = b.D == 2 ? w.d : b.dir0;
    w.v = b.nodes ? b.nodes[w.i] : b.base + w.i;
    return w;
}

// deg[d * rows + i] += the stored row of every row-pointer triple; seg_b / seg_len (nullable together: no entry tier in this call)
// as ee_segment_kernel, a row-pointer segment of length 0
__global__ __launch_bounds__(256) void dg_segment_kernel(DgBatch b, u32 nseg, u32* __restrict__ seg_b, u32* __restrict__ seg_len,
                                                        u64* __restrict__ deg, u64* __restrict__ total) {
    const u64 s64 = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 len = 0;
    if (s64 < nseg) {
        const u32 s = (u32)s64;
        const DgWalk w = dg_walk(b, s);
        const EeType& y = b.ty[w.t];
        u32 beg = 0, end = 0;
        if ((b.fast[w.in] >> w.t) & 1ull) {
            if (w.l == 0) {
                row_range(w.in ? y.tm : y.m, w.v, beg, end);
                if (end > beg) atomicAdd((unsigned long long*)&deg[(size_t)w.d * b.rows + w.i], (unsigned long long)(end - beg));
            }
            beg = end = 0;
        } else {
            row_range(w.in ? (w.l ? y.tdp : y.tm) : (w.l ? y.dp : y.m), w.v, beg, end);
        }
        len = end - beg;
        if (seg_len) {
            seg_b[s] = beg;
            seg_len[s] = len;
        }
    } else if (s64 == nseg && seg_len) {
        seg_len[nseg] = 0u;
    }
    ee_add(len, total);
}

// cnt: [0] pairs that hold MULTI_EDGE without a table row [1] entries walked outgoing [2] incoming [3] multi-edge pairs met
// [4] longest list
__global__ __launch_bounds__(256) void dg_count_kernel(DgBatch b, const u32* __restrict__ seg_b, const u32* __restrict__ seg_off,
                                                      const u32* __restrict__ wordrow, u32 n_ent, u64* __restrict__ deg,
                                                      u32* __restrict__ cnt) {
    const u64 e64 = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool live = e64 < n_ent;
    bool inw = false, missing = false, multi = false;
    u32 c = 0, key = ~0u;   // key: the counter of the entry's (position, direction); ~0u on the lanes past the last entry
    if (live) {
        const u32 e = (u32)e64;
        const u32 s = entry_vec(seg_off, wordrow, e);
        const DgWalk w = dg_walk(b, s);
        const EeType& y = b.ty[w.t];
        const u32 q = seg_b[s] + (e - seg_off[s]);
        key = w.d * b.rows + w.i;
        inw = w.in != 0;
        bool valid;
        u32 ms, md;
        u64 v = 0;
        if (!inw) {
            ms = w.v;
            md = (w.l ? y.dp : y.m).colidx[q];
            if (w.l) {
                v = y.dpval[q];
                valid = true;
            } else {
                valid = probe(y.dp, ms, md) == ~0u && probe(y.dm, ms, md) == ~0u;   // (a shadowed pair is the dp entry's)
                v = y.mval[q];
            }
        } else {
            md = w.v;
            ms = (w.l ? y.tdp : y.tm).colidx[q];
            const bool hidden = probe(y.tdm, md, ms) != ~0u;
            valid = w.l ? (hidden || probe(y.tm, md, ms) == ~0u) : !hidden;   // (a pair in both layers is the base entry's)
            if (valid) valid = ee_value(y, ms, md, v);
        }
        if (valid) {
            c = 1;
            if (v == FGPU_MULTI_EDGE) {
                const u32 r = find(y.mkey, 0u, y.n_multi, ((u64)ms << 32) | md);
                if (r == ~0u) {
                    missing = true;
                    c = 0;
                } else {
                    multi = true;
                    c = y.moff[r + 1] - y.moff[r];
                }
            }
        }
    }
    // the sum of every run of equal keys ends up on the run's first lane: step o adds the lane o further on while it is of the
    // same run (runs are consecutive lanes, so whatever lies between is of the run too)
    const u32 lane = lane_id();
    u64 sum = c;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const u64 up = __shfl_down(sum, o, WAVE);
        const u32 ku = __shfl_down(key, o, WAVE);
        if (lane + o < WAVE && ku == key) sum += up;
    }
    const u32 kprev = __shfl_up(key, 1, WAVE);
    if (live && sum && (lane == 0 || kprev != key)) atomicAdd((unsigned long long*)&deg[key], (unsigned long long)sum);
    if (__ballot(multi) != 0ull) {   // the longest list of the wavefront (wave-uniform branch): one atomicMax, not one per pair
        u32 mx = multi ? c : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (u32)__shfl_xor(mx, o, WAVE));
        if (lane == 0) atomicMax(cnt + 4, mx);
    }
    count_if(missing, cnt + 0);
    count_if(live && !inw, cnt + 1);
    count_if(live && inw, cnt + 2);
    count_if(multi, cnt + 3);
}

static fgpu_info node_degrees_impl(fgpu_ctx* ctx, const u64* nodes, u64 k, const fgpu_mat* const* m, const fgpu_mat* const* dp,
                                   const fgpu_mat* const* dm, const fgpu_mat* const* mt_m, const fgpu_mat* const* mt_dp,
                                   const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi, int n_types, int flags,
                                   u64* out_degree, u64* in_degree, u64* stats) {
    const char* fn = "fgpu_node_degrees";
    FGPU_REQUIRE(ctx, FGPU_NULL_POINTER, "%s: NULL context", fn);
    FGPU_REQUIRE(flags != 0 && (flags & ~(FGPU_DEGREE_OUT | FGPU_DEGREE_IN)) == 0, FGPU_INVALID,
                 "%s: flags %d are not FGPU_DEGREE_OUT, FGPU_DEGREE_IN or both", fn, flags);
    const bool want_out = flags & FGPU_DEGREE_OUT, want_in = flags & FGPU_DEGREE_IN;
    FGPU_REQUIRE(k == 0 || ((!want_out || out_degree) && (!want_in || in_degree)), FGPU_NULL_POINTER,
                 "%s: NULL result array for a direction the flags ask for", fn);
    FGPU_REQUIRE(n_types == 0 || m, FGPU_NULL_POINTER, "%s: NULL m", fn);
    FGPU_REQUIRE(n_types >= 0 && n_types <= EE_MAX_TYPES, FGPU_INVALID, "%s: %d types (at most %d)", fn, n_types, EE_MAX_TYPES);
    FGPU_REQUIRE(!nodes || k <= EE_MAX_ROWS, FGPU_INVALID, "%s: %llu nodes in one batch (at most %llu)", fn, (unsigned long long)k,
                 (unsigned long long)EE_MAX_ROWS);
    // ---- the layers ------------------------------------------------------------------------------------------------------
    u64 n = 0;
    bool any_dp = false;
    std::vector<EeType> hty;
    if (n_types) {
        FGPU_TRY(ee_types(fn, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, hty, n, any_dp));
        if (want_in)
            for (int t = 0; t < n_types; ++t)
                FGPU_REQUIRE(ee_at(mt_m, t), FGPU_INVALID, "%s: FGPU_DEGREE_IN walks incoming entries and mt_m[%d] is missing", fn, t);
        FGPU_REQUIRE(nodes || k == n, FGPU_INVALID, "%s: the whole-graph form takes k = the dimension %llu, not %llu", fn,
                     (unsigned long long)n, (unsigned long long)k);
    }   // (without a type there is no dimension to hold ids or k to: every position answers 0)
    // ---- the positions ---------------------------------------------------------------------------------------------------
    std::vector<u32> n32;
    if (nodes && n_types) {
        n32.resize(k);
        for (u64 i = 0; i < k; ++i) {
            FGPU_REQUIRE(nodes[i] < n, FGPU_INVALID, "%s: position %llu names node %llu, at or past %llu", fn, (unsigned long long)i,
                         (unsigned long long)nodes[i], (unsigned long long)n);
            n32[i] = (u32)nodes[i];
        }
    }
    if (k == 0) return FGPU_OK;
    if (n_types == 0) {
        if (want_out) memset(out_degree, 0, k * sizeof(u64));
        if (want_in) memset(in_degree, 0, k * sizeof(u64));
        return FGPU_OK;
    }
    // ---- tiers and windows -----------------------------------------------------------------------------------------------
    DgBatch b;
    b.D = (want_out && want_in) ? 2u : 1u;
    b.T = (u32)n_types;
    b.dir0 = want_out ? 0u : 1u;
    b.fast[0] = b.fast[1] = 0;
    u64 n_fast = 0, n_slow = 0;
    bool slow_dp = false;
    for (int t = 0; t < n_types; ++t) {
        const EeType& y = hty[t];
        const bool table = y.n_multi != 0;
        if (want_out) {
            const bool f = !y.dp.rowptr && !y.dm.rowptr && !table;
            if (f) b.fast[0] |= 1ull << t;
            else slow_dp = slow_dp || y.dp.rowptr != nullptr;
            ++(f ? n_fast : n_slow);
        }
        if (want_in) {
            const bool f = !y.tdp.rowptr && !y.tdm.rowptr && !table;
            if (f) b.fast[1] |= 1ull << t;
            else slow_dp = slow_dp || y.tdp.rowptr != nullptr;
            ++(f ? n_fast : n_slow);
        }
    }
    b.L = slow_dp ? 2u : 1u;
    const u64 per_row = (u64)b.D * b.T * b.L;
    u64 window = std::min<u64>((u64)ctx->opt.degree_window_rows, ((1ull << 31) - 1) / per_row);   // per_row <= 256
    window = std::min(window, k);
    hipStream_t st = ctx->stream();
    DevBuf<u32> dnodes, seg_b, seg_off, tot, wr_seg;
    DevBuf<EeType> dty;
    DevBuf<u64> deg;
    FGPU_TRY(dty.alloc(ctx, (size_t)n_types));
    FGPU_TRY(deg.alloc(ctx, window * b.D));
    FGPU_TRY(tot.alloc(ctx, 8));   // [0..1] entries of the window's segments (a 64-bit sum), [2..6] dg_count_kernel's cnt
    if (n_slow) {
        FGPU_TRY(seg_b.alloc(ctx, window * per_row));
        FGPU_TRY(seg_off.alloc(ctx, window * per_row + 1));
    }
    {
        ProfScope up(ctx, "dg_h2d", (nodes ? k * 4 : 0) + (size_t)n_types * sizeof(EeType));
        if (nodes) {
            FGPU_TRY(dnodes.alloc(ctx, k));
            FGPU_TRY(ctx->h2d(dnodes.p, n32.data(), k * sizeof(u32)));
        }
        FGPU_TRY(ctx->h2d(dty.p, hty.data(), (size_t)n_types * sizeof(EeType)));
    }
    b.ty = dty.p;
    u64 s_out = 0, s_in = 0, walked_out = 0, walked_in = 0, met = 0, longest = 0, windows = 0;
    for (u64 base = 0; base < k; base += window) {
        const u64 rows = std::min(window, k - base);
        b.nodes = nodes ? dnodes.p + base : nullptr;
        b.base = nodes ? 0u : (u32)base;
        b.rows = (u32)rows;
        const u32 nseg = (u32)(rows * per_row);
        FGPU_HIP(hipMemsetAsync(deg.p, 0, rows * b.D * sizeof(u64), st));
        FGPU_HIP(hipMemsetAsync(tot.p, 0, 8 * sizeof(u32), st));
        {
            ProfScope prof(ctx, "dg_segments", (u64)nseg * (n_slow ? 16 : 8));
            FGPU_TRY(launch(dg_segment_kernel, dim3(cdiv((u64)nseg + 1, 256)), dim3(256), 0, st, b, nseg, seg_b.p, seg_off.p, deg.p,
                            (u64*)tot.p));
        }
        if (n_slow) {
            u32 h[7];
            FGPU_TRY(read_words(ctx, tot.p, 2, h));
            const u64 n_ent64 = (u64)h[0] | ((u64)h[1] << 32);
            FGPU_REQUIRE(n_ent64 < 0xFFFFFFFFull, FGPU_INVALID,
                         "%s: a window of %llu positions walks %llu stored entries, past the 32-bit position space (lower degree_window_rows)",
                         fn, (unsigned long long)rows, (unsigned long long)n_ent64);
            const u32 n_ent = (u32)n_ent64;
            if (n_ent) {
                FGPU_TRY(scan_u32(ctx, seg_off.p, seg_off.p, (u64)nseg + 1, nullptr));
                FGPU_TRY(wordrow_build(ctx, seg_off.p, nseg, n_ent, wr_seg));
                {
                    ProfScope prof(ctx, "dg_count", (u64)n_ent * 16);   // (plus one 64-byte line per probe step, as ee_gather)
                    FGPU_TRY(launch(dg_count_kernel, dim3(cdiv(n_ent, 256)), dim3(256), 0, st, b, (const u32*)seg_b.p,
                                    (const u32*)seg_off.p, (const u32*)wr_seg.p, n_ent, deg.p, tot.p + 2));
                }
                FGPU_TRY(read_words(ctx, tot.p, 7, h));
                FGPU_REQUIRE(h[2] == 0, FGPU_INVALID, "%s: %u visited pairs hold MULTI_EDGE in a tensor, and its table has no row for them",
                             fn, h[2]);
                walked_out += h[3];
                walked_in += h[4];
                met += h[5];
                longest = std::max<u64>(longest, h[6]);
            }
        }
        {
            ProfScope prof(ctx, "dg_readback", rows * b.D * 8);
            if (want_out) FGPU_TRY(ctx->d2h(out_degree + base, deg.p, rows * sizeof(u64)));
            if (want_in) FGPU_TRY(ctx->d2h(in_degree + base, deg.p + (b.D == 2 ? rows : 0), rows * sizeof(u64)));
        }
        for (u64 i = 0; i < rows; ++i) {
            if (want_out) s_out += out_degree[base + i];
            if (want_in) s_in += in_degree[base + i];
        }
        ++windows;
    }
    if (stats) {
        stats[0] = k * n_fast;
        stats[1] = walked_out;
        stats[2] = walked_in;
        stats[3] = met;
        stats[4] = longest;
        stats[5] = s_out;
        stats[6] = s_in;
        stats[7] = windows;
    }
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_node_degrees(fgpu_ctx* ctx, const uint64_t* nodes, uint64_t k, const fgpu_mat* const* m,
                                       const fgpu_mat* const* dp, const fgpu_mat* const* dm, const fgpu_mat* const* mt_m,
                                       const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm, const fgpu_multi* const* multi,
                                       int n_types, int flags, uint64_t* out_degree, uint64_t* in_degree, uint64_t stats[8]) {
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    return node_degrees_impl(ctx, nodes, k, m, dp, dm, mt_m, mt_dp, mt_dm, multi, n_types, flags, out_degree, in_degree, stats);
}
