// cdlp.hip — algo.labelPropagation's numeric core: LAGraph_cdlp (called from graph/src/runtime/functions/algo_procedures.rs:1168-1270
// through lagraphx_bindings.rs:218-223) over a symmetric pattern S.  Synchronous label propagation as LDBC Graphalytics defines
// CDLP (the rules are restated in include/fgpu.h): label_0[v] = v; label_t[v] = the most frequent label_{t-1} among the stored
// entries of v's row whose column is active, ties to the smallest label; a row without a voting entry keeps its label; the run
// ends after itermax iterations or after the first one that changes nothing.
//
// The hot loop is a segmented mode.  Rows are classed ONCE per call (cdlp_count_kernel / cdlp_fill_kernel build one list per
// class), and every iteration runs one kernel per class over label_{t-1} (read only) into label_t (every vertex written once):
//   small  inactive vertices and rows of <= 2 entries: closed forms (keep / the neighbour's label / the smaller of the two)
//   short  rows of 3..64 entries, a group of 8, 16, 32 or 64 lanes per row by length: the gathered labels (NONE for an inactive
//          column) sorted across the lanes by the __shfl_xor bitonic network, run heads by a ballot, run lengths from the next
//          head, the winner a group-wide max of (length << 32) | (NONE - label) — the longest run, then the smallest label
//   mid    rows of 65..HUB_DEG - 1 entries, a workgroup per row: bitonic sort in 16 KiB of LDS, run lengths by a binary search
//          for the end of the run, the same packed key through one LDS atomicMax
//   hub    rows of HUB_DEG entries and more, by the snapshot's hub_chunks triples (mat_finalize), in three launches:
//          cdlp_hub_encode_kernel sorts a chunk's labels in LDS, run-length encodes them and folds every (label, length) pair
//          into the row's count table (open addressing over 2 x the row's entries, atomicCAS on the key word, atomicAdd on the
//          count word); cdlp_hub_reduce_kernel reduces a chunk's share of the table to the packed key and atomicMax-es it into
//          the row's word; cdlp_hub_pick_kernel writes the row's label.  The scratch is 2 x 8 bytes per hub ENTRY plus a word
//          per chunk, cleared by one kernel per iteration; no kernel depends on a row fitting in LDS.  The encode step before
//          the atomics is what keeps the steady state (a hub whose neighbours nearly all carry one label) from issuing one
//          atomic per entry on a single word.
//
// Concurrency rules (per-XCD L2s are not coherent inside a launch; MI355X_MICROARCH.md):
//   - inside a launch label_{t-1} is only read and every word of label_t is written by exactly one thread: no kernel reads a
//     word another workgroup of the same launch writes;
//   - the hub count table is touched inside a launch only through atomicCAS / atomicAdd / atomicMax (device scope); plain loads
//     of it happen in the NEXT launch (reduce after encode, pick after reduce);
//   - all ordering between the classes, the hub passes and the iterations is by kernel boundaries on the context's stream.
//     Nothing polls or spins;
//   - every iteration kernel adds its changed labels into chg[j] (block_add_u64) and returns at once when chg[j - 1] == 0, i.e.
//     when the previous iteration changed nothing: the host launches CDLP_BATCH iterations at a time and reads the counters
//     back once per batch.  After an iteration that changed nothing both buffers hold the same labels, so the parity of the
//     skipped launches is harmless.
// Static LDS: 16 KiB + a few words (mid, hub encode); no dynamic LDS.
#include "algo.hpp"

namespace fgpu {

constexpr u32 CDLP_NONE = 0xFFFFFFFFu;   // no label (check_adjacency keeps vertex ids below it): pads sort to the end
constexpr u32 CDLP_BATCH = 4;            // iterations launched per read-back of the changed counters
constexpr u32 CDLP_BINS = 5;             // lists: short rows by group width 8 / 16 / 32 / 64, then the mid rows
constexpr u32 CDLP_SHORT_MAX = 64;
constexpr u32 CDLP_LDS = HUB_CHUNK;      // labels a workgroup sorts in LDS (16 KiB): a mid row, or one hub chunk
static_assert(HUB_DEG <= CDLP_LDS && HUB_CHUNK <= CDLP_LDS, "a mid row and a hub chunk must fit the LDS sort");

struct CdlpLists {
    const u32* rows;            // the five lists, back to back
    u32 off[CDLP_BINS + 1];
};

// class of row v: 0 small (closed form, or not active), 1-4 short by group width, 5 mid, 6 hub
__device__ __forceinline__ u32 cdlp_bin(u32 deg, bool on) {
    if (deg >= HUB_DEG) return 6u;
    if (!on || deg <= 2u) return 0u;
    if (deg <= 8u) return 1u;
    if (deg <= 16u) return 2u;
    if (deg <= 32u) return 3u;
    if (deg <= CDLP_SHORT_MAX) return 4u;
    return 5u;
}

__device__ __forceinline__ u32 cdlp_vote(const u32* __restrict__ in, const u64* __restrict__ act, u32 w) {
    return vertex_on(act, w) ? in[w] : CDLP_NONE;
}

// the label a packed winner stands for (0: no entry voted, the row keeps `keep`)
__device__ __forceinline__ u32 cdlp_unpack(unsigned long long best, u32 keep) {
    return best ? CDLP_NONE - (u32)(best & 0xFFFFFFFFull) : keep;
}

__global__ __launch_bounds__(256) void cdlp_init_kernel(u32* __restrict__ lab, u32 n) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) lab[v] = v;
}

// cnt[b - 1] += rows of bin b (1..5), cnt[5] += entries of hub rows, cnt[6] += entries of active rows
__global__ __launch_bounds__(256) void cdlp_count_kernel(const u32* __restrict__ rowptr, const u64* __restrict__ act, u32 n,
                                                        unsigned long long* cnt) {
    u64 c[CDLP_BINS] = {0, 0, 0, 0, 0}, hub = 0, ent = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const u32 deg = rowptr[v + 1] - rowptr[v];
        const bool on = vertex_on(act, v);
        const u32 b = cdlp_bin(deg, on);
#pragma unroll
        for (u32 k = 0; k < CDLP_BINS; ++k) c[k] += b == k + 1 ? 1u : 0u;
        if (b == 6u) hub += deg;
        if (on) ent += deg;
    }
#pragma unroll
    for (u32 k = 0; k < CDLP_BINS; ++k) block_add_u64(c[k], &cnt[k]);
    block_add_u64(hub, &cnt[5]);
    block_add_u64(ent, &cnt[6]);
}

// the lists themselves: one atomic per wavefront and bin (the order inside a list does not matter)
__global__ __launch_bounds__(256) void cdlp_fill_kernel(const u32* __restrict__ rowptr, const u64* __restrict__ act, u32 n,
                                                       CdlpLists ls, u32* __restrict__ rows, u32* cursor) {
    const u32 lane = lane_id();
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += (u64)gridDim.x * 256) {
        const u64 v = base + threadIdx.x;
        u32 b = 0;
        if (v < n) b = cdlp_bin(rowptr[v + 1] - rowptr[v], vertex_on(act, (u32)v));
#pragma unroll
        for (u32 k = 1; k <= CDLP_BINS; ++k) {
            const u64 m = __ballot(b == k);
            if (!m) continue;
            const u32 first = (u32)__builtin_ctzll(m);
            u32 at = 0;
            if (lane == first) at = atomicAdd(&cursor[k - 1], (u32)__builtin_popcountll(m));
            at = __shfl(at, first, 64);
            if (b == k) rows[ls.off[k - 1] + at + wave_slot(m, lane)] = (u32)v;
        }
    }
}

// small: inactive vertices keep their word; rows of <= 2 entries by closed form
__global__ __launch_bounds__(256) void cdlp_small_kernel(CsrView a, const u64* __restrict__ act, const u32* __restrict__ in,
                                                        u32* __restrict__ out, u32 n, const unsigned long long* prev,
                                                        unsigned long long* chg) {
    if (prev && *prev == 0ull) return;
    u64 changed = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const u32 b = a.rowptr[v], deg = a.rowptr[v + 1] - b;
        const bool on = vertex_on(act, v);
        if (cdlp_bin(deg, on) != 0u) continue;
        const u32 l = in[v];
        u32 nl = l;
        if (on && deg) {
            const u32 x = cdlp_vote(in, act, a.colidx[b]);
            const u32 y = deg == 2u ? cdlp_vote(in, act, a.colidx[b + 1]) : CDLP_NONE;
            const u32 m = x < y ? x : y;   // one vote: that label; two: equal, or a tie of one each that goes to the smaller
            if (m != CDLP_NONE) nl = m;
        }
        out[v] = nl;
        changed += nl != l ? 1u : 0u;
    }
    block_add_u64(changed, chg);
}

// short: a group of G lanes per row of at most G entries
template <u32 G>
__global__ __launch_bounds__(256) void cdlp_short_kernel(CsrView a, const u64* __restrict__ act, const u32* __restrict__ in,
                                                        u32* __restrict__ out, const u32* __restrict__ rows, u32 count,
                                                        const unsigned long long* prev, unsigned long long* chg) {
    if (prev && *prev == 0ull) return;
    constexpr u32 RPW = 64 / G;   // rows per wavefront
    const u32 lane = lane_id();
    const u32 p = lane & (G - 1), gbase = lane & ~(G - 1);
    const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6;
    const u64 nwaves = ((u64)gridDim.x * 256) >> 6;
    const u64 gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    u64 changed = 0;
    for (u64 i0 = wave * RPW; i0 < count; i0 += nwaves * RPW) {   // (wave-uniform trip count: every lane takes the shuffles)
        const u64 i = i0 + (gbase / G);
        const bool have = i < count;
        u32 v = 0, b = 0, deg = 0;
        if (have) { v = rows[i]; b = a.rowptr[v]; deg = a.rowptr[v + 1] - b; }
        u32 x = p < deg ? cdlp_vote(in, act, a.colidx[b + p]) : CDLP_NONE;
#pragma unroll
        for (u32 k = 2; k <= G; k <<= 1) {
#pragma unroll
            for (u32 j = k >> 1; j > 0; j >>= 1) {
                const u32 y = __shfl_xor(x, (int)j, 64);
                const bool up = (p & k) == 0;          // ascending block
                const bool low = (p & j) == 0;         // this lane holds the lower slot of the pair
                const u32 mn = x < y ? x : y, mx = x < y ? y : x;
                x = (low == up) ? mn : mx;
            }
        }
        const u32 before = __shfl_up(x, 1, 64);
        const bool head = p == 0 || before != x;       // pads form one last run that only bounds the run before it
        const u64 heads = (__ballot(head) >> gbase) & gmask;
        const u64 later = p + 1 < 64 ? heads >> (p + 1) : 0ull;
        const u32 next = later ? p + 1 + (u32)__builtin_ctzll(later) : G;
        unsigned long long key = (head && x != CDLP_NONE) ? ((unsigned long long)(next - p) << 32) | (CDLP_NONE - x) : 0ull;
#pragma unroll
        for (u32 d = G >> 1; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, (int)d, 64);
            key = o > key ? o : key;
        }
        if (have && p == 0) {
            const u32 l = in[v], nl = cdlp_unpack(key, l);
            out[v] = nl;
            changed += nl != l ? 1u : 0u;
        }
    }
    block_add_u64(changed, chg);
}

// ascending bitonic sort of s[0, P), P a power of two >= 2, by the 256 threads of a workgroup (s filled and a barrier passed
// on entry; ends in a barrier)
__device__ __forceinline__ void cdlp_sort_lds(u32* s, u32 P) {
    const u32 t = threadIdx.x;
    for (u32 k = 2; k <= P; k <<= 1) {
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 i = t; i < (P >> 1); i += 256) {
                const u32 lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const u32 x = s[lo], y = s[hi];
                if ((x > y) == ((lo & k) == 0)) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    }
}

// entries [b, e) of the matrix as votes into s, padded to the power of two P the function returns; sorted on return
__device__ __forceinline__ u32 cdlp_load_sorted(u32* s, const u32* __restrict__ col, const u64* __restrict__ act,
                                                const u32* __restrict__ in, u32 b, u32 e) {
    const u32 len = e - b;
    const u32 P = len <= 2u ? 2u : 1u << (32 - __clz((int)(len - 1)));
    for (u32 i = threadIdx.x; i < P; i += 256) s[i] = i < len ? cdlp_vote(in, act, col[b + i]) : CDLP_NONE;
    __syncthreads();
    cdlp_sort_lds(s, P);
    return P;
}

// length of the run of s[p] that starts at p in the sorted s[0, P)
__device__ __forceinline__ u32 cdlp_run_length(const u32* s, u32 P, u32 p) {
    const u32 x = s[p];
    u32 lo = p + 1, hi = P;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (s[mid] == x) lo = mid + 1; else hi = mid;
    }
    return lo - p;
}

// mid: a workgroup per row
__global__ __launch_bounds__(256) void cdlp_mid_kernel(CsrView a, const u64* __restrict__ act, const u32* __restrict__ in,
                                                      u32* __restrict__ out, const u32* __restrict__ rows, u32 count,
                                                      const unsigned long long* prev, unsigned long long* chg) {
    if (prev && *prev == 0ull) return;
    __shared__ u32 s[CDLP_LDS];
    __shared__ unsigned long long best;
    u64 changed = 0;
    for (u32 it = blockIdx.x; it < count; it += gridDim.x) {
        const u32 v = rows[it];
        const u32 b = a.rowptr[v], e = a.rowptr[v + 1];   // 64 < e - b < HUB_DEG <= CDLP_LDS (cdlp_bin)
        if (threadIdx.x == 0) best = 0ull;
        const u32 P = cdlp_load_sorted(s, a.colidx, act, in, b, e);
        for (u32 p = threadIdx.x; p < P; p += 256) {
            const u32 x = s[p];
            if (x != CDLP_NONE && (p == 0 || s[p - 1] != x))
                atomicMax(&best, ((unsigned long long)cdlp_run_length(s, P, p) << 32) | (CDLP_NONE - x));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 l = in[v], nl = cdlp_unpack(best, l);
            out[v] = nl;
            changed += nl != l ? 1u : 0u;
        }
        __syncthreads();   // s and best are reused by the next row
    }
    block_add_u64(changed, chg);
}

// ---- hub rows -------------------------------------------------------------------------------------------------------------
// Chunk h = (row, cb, ce) of the snapshot's list; the chunks of a row are consecutive in it and cb = rowptr[row] + k HUB_CHUNK
// (hub_scan_kernel), so the row's first chunk is h - k.  coff[h] = hub entries in the chunks before h: the row's table starts
// at slot 2 (coff[h] - (cb - rowptr[row])) and has 2 deg(row) slots; best[h - k] is the row's packed winner.
struct CdlpHub {
    const u32* chunks;
    u32 n_chunks;
    const u32* coff;
    unsigned long long* best;   // n_chunks words
    u32* keys;                  // 2 H slots: label + 1, 0 = free
    u32* cnts;                  // 2 H slots
};

__global__ __launch_bounds__(256) void cdlp_chunk_len_kernel(const u32* __restrict__ chunks, u32 n_chunks, u32* __restrict__ len) {
    for (u32 h = blockIdx.x * blockDim.x + threadIdx.x; h < n_chunks; h += gridDim.x * blockDim.x)
        len[h] = chunks[3 * h + 2] - chunks[3 * h + 1];
}

__global__ __launch_bounds__(256) void cdlp_clear_kernel(unsigned long long* __restrict__ p, u64 words, const unsigned long long* prev) {
    if (prev && *prev == 0ull) return;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < words; i += (u64)gridDim.x * 256) p[i] = 0ull;
}

__global__ __launch_bounds__(256) void cdlp_hub_encode_kernel(CdlpHub hb, const u32* __restrict__ rowptr, const u32* __restrict__ col,
                                                             const u64* __restrict__ act, const u32* __restrict__ in,
                                                             const unsigned long long* prev) {
    if (prev && *prev == 0ull) return;
    __shared__ u32 s[CDLP_LDS];
    for (u32 h = blockIdx.x; h < hb.n_chunks; h += gridDim.x) {
        const u32 row = hb.chunks[3 * h], cb = hb.chunks[3 * h + 1], ce = hb.chunks[3 * h + 2];   // ce - cb <= HUB_CHUNK <= CDLP_LDS
        if (!vertex_on(act, row)) continue;   // (workgroup-uniform)
        const u32 rs = rowptr[row];
        const u32 tsize = 2u * (rowptr[row + 1] - rs);
        const u64 toff = 2ull * (u64)(hb.coff[h] - (cb - rs));
        u32* keys = hb.keys + toff;
        u32* cnts = hb.cnts + toff;
        const u32 P = cdlp_load_sorted(s, col, act, in, cb, ce);
        for (u32 p = threadIdx.x; p < P; p += 256) {
            const u32 x = s[p];
            if (x == CDLP_NONE || (p != 0 && s[p - 1] == x)) continue;
            const u32 len = cdlp_run_length(s, P, p);
            // at most deg(row) distinct labels meet 2 deg(row) slots: a free or matching slot always turns up
            u32 slot = (u32)(((u64)(x * 0x9E3779B1u) * tsize) >> 32);
            for (;;) {
                const u32 k = atomicCAS(&keys[slot], 0u, x + 1u);
                if (k == 0u || k == x + 1u) { atomicAdd(&cnts[slot], len); break; }
                slot = slot + 1u == tsize ? 0u : slot + 1u;
            }
        }
        __syncthreads();   // s is reused by the next chunk
    }
}

// a chunk reduces slots [2 (cb - rs), 2 (ce - rs)) of its row's table
__global__ __launch_bounds__(256) void cdlp_hub_reduce_kernel(CdlpHub hb, const u32* __restrict__ rowptr, const u64* __restrict__ act,
                                                             const unsigned long long* prev) {
    if (prev && *prev == 0ull) return;
    for (u32 h = blockIdx.x; h < hb.n_chunks; h += gridDim.x) {
        const u32 row = hb.chunks[3 * h], cb = hb.chunks[3 * h + 1], ce = hb.chunks[3 * h + 2];
        if (!vertex_on(act, row)) continue;
        const u32 rs = rowptr[row];
        const u64 toff = 2ull * (u64)(hb.coff[h] - (cb - rs));
        const u32* keys = hb.keys + toff;
        const u32* cnts = hb.cnts + toff;
        unsigned long long key = 0ull;
        for (u32 i = 2u * (cb - rs) + threadIdx.x; i < 2u * (ce - rs); i += 256) {
            const u32 k = keys[i];
            if (k) {
                const unsigned long long c = ((unsigned long long)cnts[i] << 32) | (CDLP_NONE - (k - 1u));
                key = c > key ? c : key;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, d, 64);
            key = o > key ? o : key;
        }
        if (lane_id() == 0 && key) atomicMax(&hb.best[h - (cb - rs) / HUB_CHUNK], key);
    }
}

__global__ __launch_bounds__(256) void cdlp_hub_pick_kernel(CdlpHub hb, const u32* __restrict__ rowptr, const u32* __restrict__ in,
                                                           u32* __restrict__ out, const unsigned long long* prev,
                                                           unsigned long long* chg) {
    if (prev && *prev == 0ull) return;
    u64 changed = 0;
    for (u32 h = blockIdx.x * blockDim.x + threadIdx.x; h < hb.n_chunks; h += gridDim.x * blockDim.x) {
        const u32 row = hb.chunks[3 * h];
        if (hb.chunks[3 * h + 1] != rowptr[row]) continue;   // the row's first chunk speaks for it
        const u32 l = in[row], nl = cdlp_unpack(hb.best[h], l);   // (an inactive row left its word 0)
        out[row] = nl;
        changed += nl != l ? 1u : 0u;
    }
    block_add_u64(changed, chg);
}

// labels -> int64 (-1 for inactive vertices); the labels in use are marked in a bitmap of n bits
__global__ __launch_bounds__(256) void cdlp_finish_kernel(const u32* __restrict__ lab, const u64* __restrict__ act, u32 n,
                                                         long long* __restrict__ out, u32* mark) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        if (!vertex_on(act, v)) { out[v] = -1; continue; }
        const u32 l = lab[v];
        out[v] = (long long)l;
        const u32 bit = 1u << (l & 31u);
        if (!(mark[l >> 5] & bit)) atomicOr(&mark[l >> 5], bit);   // (a stale 0 only repeats the atomic)
    }
}

__global__ __launch_bounds__(256) void cdlp_popcount_kernel(const u32* __restrict__ mark, u32 words, unsigned long long* dst) {
    u64 c = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) c += (u32)__popc(mark[i]);
    block_add_u64(c, dst);
}

template <u32 G>
static fgpu_info cdlp_launch_short(fgpu_ctx* ctx, CsrView a, const u64* act, const u32* in, u32* out, const u32* rows, u32 count,
                                   const unsigned long long* prev, unsigned long long* chg) {
    if (!count) return FGPU_OK;
    return launch(cdlp_short_kernel<G>, dim3(capped_grid(ctx, count, 256 / G, 8)), dim3(256), 0, ctx->stream(), a, act, in, out,
                  rows, count, prev, chg);
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_cdlp(fgpu_ctx* ctx, const fgpu_mat* S, const uint64_t* active_bitmap, int32_t itermax, int64_t* label,
                               uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && S && label, FGPU_NULL_POINTER, "fgpu_cdlp: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_cdlp", S, nullptr));
    FGPU_REQUIRE(itermax >= 0, FGPU_INVALID, "fgpu_cdlp: itermax must not be negative");
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)S->nrows;
    if (n == 0) return FGPU_OK;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, S));
    FGPU_TRY(mat_ensure_finalized(S));   // the hub lists
    hipStream_t st = ctx->stream();
    DevBuf<u64> act;
    DevBuf<u32> lab, rows, cursor, clen, coff, mark;
    DevBuf<unsigned long long> cnt, chg, hubmem;
    DevBuf<long long> wide;
    if (active_bitmap) FGPU_TRY(upload_active(ctx, act, active_bitmap, n));
    const u64* a = act.p;
    const CsrView sv = view_of(S);
    const u32 mark_words = cdiv(n, 32);
    FGPU_TRY(lab.alloc(ctx, 2 * (size_t)n));
    FGPU_TRY(cnt.alloc(ctx, 8));   // bins 1..5, hub entries, entries of active rows, distinct labels
    FGPU_TRY(chg.alloc(ctx, CDLP_BATCH));
    FGPU_TRY(wide.alloc(ctx, n));
    FGPU_TRY(mark.alloc(ctx, mark_words));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, 8 * sizeof(unsigned long long), st));
    FGPU_HIP(hipMemsetAsync(mark.p, 0, (size_t)mark_words * sizeof(u32), st));
    const u32 vgrid = capped_grid(ctx, n, 256, 8);
    FGPU_TRY(launch(cdlp_init_kernel, dim3(vgrid), dim3(256), 0, st, lab.p, n));
    u32* buf[2] = {lab.p, lab.p + n};
    u64 iters = 0, changed_last = 0, row_entries = 0;
    u32 cur = 0;   // buf[cur] holds the labels
    if (itermax > 0) {
        // the classes, once per call
        FGPU_TRY(launch(cdlp_count_kernel, dim3(vgrid), dim3(256), 0, st, sv.rowptr, a, n, cnt.p));
        unsigned long long hc[7];
        FGPU_TRY(ctx->d2h(hc, cnt.p, sizeof(hc)));
        row_entries = hc[6];
        CdlpLists ls;
        ls.off[0] = 0;
        for (u32 k = 0; k < CDLP_BINS; ++k) ls.off[k + 1] = ls.off[k] + (u32)hc[k];
        FGPU_TRY(rows.alloc(ctx, ls.off[CDLP_BINS]));
        ls.rows = rows.p;
        if (ls.off[CDLP_BINS]) {
            FGPU_TRY(cursor.alloc(ctx, CDLP_BINS));
            FGPU_HIP(hipMemsetAsync(cursor.p, 0, CDLP_BINS * sizeof(u32), st));
            FGPU_TRY(launch(cdlp_fill_kernel, dim3(vgrid), dim3(256), 0, st, sv.rowptr, a, n, ls, rows.p, cursor.p));
        }
        CdlpHub hb = {};
        const u32 nch = S->n_hub_chunks;
        const u64 hub_entries = hc[5];
        const u64 hub_words = (u64)nch + 2 * hub_entries;   // best[nch]; keys and counts, 2 H u32 each
        if (nch) {
            FGPU_TRY(clen.alloc(ctx, nch));
            FGPU_TRY(coff.alloc(ctx, nch));
            FGPU_TRY(hubmem.alloc(ctx, hub_words));
            FGPU_TRY(launch(cdlp_chunk_len_kernel, dim3(capped_grid(ctx, nch, 256, 8)), dim3(256), 0, st,
                            (const u32*)S->hub_chunks.p, nch, clen.p));
            FGPU_TRY(scan_u32(ctx, clen.p, coff.p, nch, nullptr));
            hb.chunks = S->hub_chunks.p;
            hb.n_chunks = nch;
            hb.coff = coff.p;
            hb.best = hubmem.p;
            hb.keys = (u32*)(hubmem.p + nch);
            hb.cnts = hb.keys + 2 * hub_entries;
        }
        const u32 hgrid = hub_grid(ctx, S);
        bool done = false;
        while (!done && iters < (u64)itermax) {
            const u32 nb = (u64)itermax - iters < CDLP_BATCH ? (u32)((u64)itermax - iters) : CDLP_BATCH;
            FGPU_HIP(hipMemsetAsync(chg.p, 0, CDLP_BATCH * sizeof(unsigned long long), st));
            for (u32 j = 0; j < nb; ++j) {
                const unsigned long long* prev = j ? chg.p + j - 1 : nullptr;
                unsigned long long* c = chg.p + j;
                const u32* src = buf[cur];
                u32* dst = buf[cur ^ 1];
                FGPU_TRY(launch(cdlp_small_kernel, dim3(vgrid), dim3(256), 0, st, sv, a, src, dst, n, prev, c));
                FGPU_TRY(cdlp_launch_short<8>(ctx, sv, a, src, dst, rows.p + ls.off[0], ls.off[1] - ls.off[0], prev, c));
                FGPU_TRY(cdlp_launch_short<16>(ctx, sv, a, src, dst, rows.p + ls.off[1], ls.off[2] - ls.off[1], prev, c));
                FGPU_TRY(cdlp_launch_short<32>(ctx, sv, a, src, dst, rows.p + ls.off[2], ls.off[3] - ls.off[2], prev, c));
                FGPU_TRY(cdlp_launch_short<64>(ctx, sv, a, src, dst, rows.p + ls.off[3], ls.off[4] - ls.off[3], prev, c));
                if (const u32 nmid = ls.off[5] - ls.off[4])
                    FGPU_TRY(launch(cdlp_mid_kernel, dim3(capped_grid(ctx, nmid, 1, 8)), dim3(256), 0, st, sv, a, src, dst,
                                    (const u32*)(rows.p + ls.off[4]), nmid, prev, c));
                if (nch) {
                    FGPU_TRY(launch(cdlp_clear_kernel, dim3(capped_grid(ctx, hub_words, 1024, 8)), dim3(256), 0, st, hubmem.p,
                                    hub_words, prev));
                    FGPU_TRY(launch(cdlp_hub_encode_kernel, dim3(hgrid), dim3(256), 0, st, hb, sv.rowptr, sv.colidx, a, src, prev));
                    FGPU_TRY(launch(cdlp_hub_reduce_kernel, dim3(hgrid), dim3(256), 0, st, hb, sv.rowptr, a, prev));
                    FGPU_TRY(launch(cdlp_hub_pick_kernel, dim3(capped_grid(ctx, nch, 256, 8)), dim3(256), 0, st, hb, sv.rowptr,
                                    src, dst, prev, c));
                }
                cur ^= 1;
            }
            u32 w[2 * CDLP_BATCH];
            FGPU_TRY(read_words(ctx, (const u32*)chg.p, 2 * CDLP_BATCH, w));   // one read-back per batch
            for (u32 j = 0; j < nb && !done; ++j) {
                changed_last = (u64)w[2 * j] | ((u64)w[2 * j + 1] << 32);
                ++iters;
                done = changed_last == 0;   // the launches behind it returned at once: both buffers hold these labels
            }
        }
    }
    FGPU_TRY(launch(cdlp_finish_kernel, dim3(vgrid), dim3(256), 0, st, (const u32*)buf[cur], a, n, wide.p, mark.p));
    FGPU_TRY(launch(cdlp_popcount_kernel, dim3(capped_grid(ctx, mark_words, 256, 8)), dim3(256), 0, st, (const u32*)mark.p,
                    mark_words, cnt.p + 7));
    FGPU_TRY(ctx->d2h(label, wide.p, (size_t)n * sizeof(int64_t)));   // one DMA when label[] is pinned
    if (stats) {
        unsigned long long distinct = 0;
        FGPU_TRY(ctx->d2h(&distinct, cnt.p + 7, sizeof(distinct)));
        stats[0] = iters;
        stats[1] = changed_last;
        stats[2] = iters * row_entries;
        stats[3] = distinct;
    }
    FGPU_HIP(hipStreamSynchronize(st));
    return FGPU_OK;
}
