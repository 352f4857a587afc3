// msf.hip — algo.MSF's numeric core: LAGraph_msf (called from graph/src/runtime/functions/algo_procedures.rs:1711-1717 through
// lagraphx_bindings.rs:261-267) over a symmetric weighted matrix W.  Boruvka over the prelude's union-find forest (algo.hpp); the rules
// (the edge order, what counts as an entry, the broken-promise guarantee) are written out in include/fgpu.h.
//
// Every unordered pair {v, w} is one edge with the key (K(bits), min, max); K (fp64_sort_key) is the IEEE totalOrder with -0.0 = +0.0
// on the stored bit pattern.  The order is strict and total, so the minimum spanning forest is unique and the kernels may race
// in any order.  A round, over comp[] = the flat parent forest of the previous round:
//   1. min weight  (valued W only) every live row reduces K over its external entries (comp[v] != comp[w], both ends active,
//      no diagonal) and issues ONE atomicMin into best_w[comp[v]]; its own minimum is kept in rowmin[v].
//   2. min pair    the live rows whose rowmin equals best_w[comp] scan again: the entries with K == best_w[comp] compete with
//      one atomicMin of (lo << 32 | hi) per row into best_e[comp].  A BOOL W (every weight 1.0) has only this pass.
//   3. hook        a thread per root with a chosen pair joins the two trees (forest_hook).  The thread whose CAS
//      turned the root `hi` into a non-root writes the pair into edge_of[hi]: a vertex stops being a root once, so the slot
//      has one writer, a mutual choice is recorded once, and an edge is recorded ONLY by a hook that joined two trees —
//      whatever W holds, the recorded pairs are a forest with (active vertices - roots) edges.
//   4. compress    pointer jumping by whole launches until a launch changes nothing.
// The run ends after the first round in which no root chose a pair (one read-back of two counters per round).
// Row classes: rows below HUB_DEG go a 64-row word per wavefront, entry-parallel over the word's contiguous entries (columns
// and values coalesced along the rows, the per-row minimum by a segmented wave scan and a 64-bit LDS min per row); rows from
// HUB_DEG up are split by the snapshot's hub chunks, a workgroup and one atomic per chunk.
// Monotone skip: a row (hub chunk) whose entries were all internal in some round is internal for ever — components only
// merge — so it is flagged in done[] (cdone[]) and never read again; stats[2] shows the effect.
// The forest leaves in (row < col) order sorted by (row, col): the recorded pairs are compacted, built into a CSR by the COO
// builder (mat_from_device_coo: its rows come out ascending and sorted), and one thread per pair probes W for the weight.
//
// Concurrency rules (per-XCD L2s are not coherent inside a launch; the forest's own are in algo.hpp):
//   - best_w / best_e are only ever lowered by atomicMin inside a launch; the plain load in front of the atomic is a filter:
//     a stale word is a LARGER one, so a skipped atomic would have changed nothing;
//   - comp[], best_w (pass 2), done[], rowmin[] are written by the launch before the one that reads them, done / rowmin words
//     by the one wavefront that owns the row word.  Nothing polls or spins; phases are separated by kernel boundaries.
// Static LDS: 5.4 KiB (row kernel); no dynamic LDS.
#include "algo.hpp"

namespace fgpu {

constexpr u64 MSF_NONE = ~0ull;
constexpr u64 MSF_ONE = 0x3FF0000000000000ull;   // 1.0

// lowers *dst to x; the plain load only filters (see the rules above)
__device__ __forceinline__ void msf_lower(u64* dst, u64 x) {
    if (*dst > x) atomicMin((unsigned long long*)dst, (unsigned long long)x);
}

// passes 1 (WPASS) and 2 over the rows shorter than HUB_DEG.  `best` is best_w in pass 1 and best_e in pass 2; `bw` is best_w
// as pass 1 left it (pass 2 of a valued W).  The pass that sees every external entry (pass 1, or the only pass of a BOOL W)
// maintains done[].
template <bool VALUED, bool WPASS>
__global__ __launch_bounds__(256) void msf_rows_kernel(CsrView a, const u64* __restrict__ vals, const u64* __restrict__ act,
                                                      const u32* __restrict__ comp, u32 n, u64* __restrict__ done,
                                                      u64* __restrict__ rowmin, const u64* __restrict__ bw, u64* best,
                                                      unsigned long long* entries) {
    constexpr bool MARKS = WPASS || !VALUED;
    __shared__ u32 s_off[4][65];   // exclusive prefix of the word's taken row lengths
    __shared__ u32 s_rb[4][64];    // first entry of each row
    __shared__ u32 s_cv[4][64];    // comp[] of each row
    __shared__ u64 s_min[4][64];   // the row's minimum key
    __shared__ u32 s_alive[4][64]; // the row has an external entry
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * 256) >> 6;
    const u32 nwords = (n + 63) >> 6;
    const u32* __restrict__ col = a.colidx;
    u32* off = s_off[wv];
    u32* rbs = s_rb[wv];
    u32* cvs = s_cv[wv];
    u64* mins = s_min[wv];
    u32* alive = s_alive[wv];
    u64 seen = 0;
    for (u32 g = wave; g < nwords; g += nwaves) {
        const u64 dn = done[g];
        const u32 v = (g << 6) + lane;
        u32 rb = 0, re = 0, cv = 0;
        if (v < n) { rb = a.rowptr[v]; re = a.rowptr[v + 1]; cv = comp[v]; }
        bool take = v < n && re > rb && re - rb < HUB_DEG && !((dn >> lane) & 1ull) && vertex_on(act, v);
        if (VALUED && !WPASS) take = take && rowmin[v] == bw[cv];
        const u64 tmask = __ballot(take);
        if (!tmask) continue;   // (wave-uniform)
        const u32 len = take ? re - rb : 0u;
        u32 inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = __shfl_up(inc, d, 64);
            if (lane >= (u32)d) inc += y;
        }
        off[lane + 1] = inc;
        if (lane == 0) off[0] = 0;
        rbs[lane] = rb;
        cvs[lane] = cv;
        mins[lane] = MSF_NONE;
        alive[lane] = 0u;
        const u32 total = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        if (lane == 0) seen += total;
        for (u32 e0 = 0; e0 < total; e0 += 64) {
            const u32 e = e0 + lane;
            const bool valid = e < total;
            u32 lo = 0, hi = 64;   // largest lo with off[lo] <= e
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const u32 mid = (lo + hi) >> 1;
                if (off[mid] <= e) lo = mid; else hi = mid;
            }
            const u32 seg = valid ? lo : 64u;
            u64 key = MSF_NONE;
            if (valid) {
                const u32 idx = rbs[lo] + (e - off[lo]);
                const u32 w = col[idx];
                const u32 rv = (g << 6) + lo;
                const u32 c = cvs[lo];
                if (w != rv && vertex_on(act, w) && comp[w] != c) {
                    const u64 pair = rv < w ? ((u64)rv << 32) | w : ((u64)w << 32) | rv;
                    if (WPASS) key = fp64_sort_key(vals[idx]);
                    else if (VALUED) key = fp64_sort_key(vals[idx]) == bw[c] ? pair : MSF_NONE;
                    else key = pair;
                    if (MARKS) alive[lo] = 1u;
                }
            }
            // the minimum of every row's run of lanes lands in the run's last lane
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u64 y = __shfl_up(key, d, 64);
                const u32 s = __shfl_up(seg, d, 64);
                if (lane >= (u32)d && s == seg && y < key) key = y;
            }
            const u32 nseg = __shfl_down(seg, 1, 64);
            if (valid && (lane == 63 || nseg != seg) && key != MSF_NONE) atomicMin((unsigned long long*)&mins[lo], key);
        }
        const u64 m = mins[lane];
        if (WPASS && take) rowmin[v] = m;
        if (take && m != MSF_NONE) msf_lower(&best[cv], m);
        if (MARKS) {
            const u64 fresh = tmask & ~__ballot(alive[lane] != 0u);
            if (lane == 0 && fresh) done[g] = dn | fresh;
        }
    }
    block_add_u64(seen, entries);
}

// the same for the rows of HUB_DEG entries and more: a workgroup and one atomic per chunk of the snapshot's hub list
template <bool VALUED, bool WPASS>
__global__ __launch_bounds__(256) void msf_hubs_kernel(const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                      const u64* __restrict__ vals, const u64* __restrict__ act,
                                                      const u32* __restrict__ comp, uint8_t* __restrict__ cdone,
                                                      u64* __restrict__ chunkmin, const u64* __restrict__ bw, u64* best,
                                                      unsigned long long* entries) {
    constexpr bool MARKS = WPASS || !VALUED;
    __shared__ u32 s_take, s_c;
    __shared__ u64 s_part[4];
    u64 seen = 0;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 row = hub[3 * h], b = hub[3 * h + 1], e = hub[3 * h + 2];
        if (threadIdx.x == 0) {
            const u32 c = comp[row];
            bool take = b < e && !cdone[h] && vertex_on(act, row);
            if (VALUED && !WPASS) take = take && chunkmin[h] == bw[c];
            s_take = take ? 1u : 0u;
            s_c = c;
        }
        __syncthreads();
        const bool take = s_take != 0;
        const u32 c = s_c;
        if (!take) { __syncthreads(); continue; }   // (workgroup-uniform)
        u64 key = MSF_NONE;
        int any = 0;
        const u64 want = (VALUED && !WPASS) ? bw[c] : 0ull;
        for (u32 i = b + threadIdx.x; i < e; i += 256) {
            const u32 w = col[i];
            if (w == row || !vertex_on(act, w) || comp[w] == c) continue;
            any = 1;
            const u64 pair = row < w ? ((u64)row << 32) | w : ((u64)w << 32) | row;
            u64 k;
            if (WPASS) k = fp64_sort_key(vals[i]);
            else if (VALUED) k = fp64_sort_key(vals[i]) == want ? pair : MSF_NONE;
            else k = pair;
            key = k < key ? k : key;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 y = __shfl_xor(key, d, 64);
            key = y < key ? y : key;
        }
        if (lane_id() == 0) s_part[threadIdx.x >> 6] = key;
        any = __syncthreads_or(any);
        if (threadIdx.x == 0) {
            u64 m = s_part[0];
            for (int k = 1; k < 4; ++k) m = s_part[k] < m ? s_part[k] : m;
            if (WPASS) chunkmin[h] = m;
            if (m != MSF_NONE) msf_lower(&best[c], m);
            if (MARKS && !any) cdone[h] = 1;
            seen += e - b;
        }
        __syncthreads();   // s_take, s_c and s_part are reused by the next chunk
    }
    if (threadIdx.x == 0 && seen) atomicAdd(entries, (unsigned long long)seen);
}

// step 3: a thread per root that chose a pair.  It clears the root's best_w / best_e for the next round (its own words) and
// records the pair where its CAS made `hi` a non-root.
__global__ __launch_bounds__(256) void msf_hook_kernel(u32* parent, u64* __restrict__ best_w, u64* __restrict__ best_e,
                                                      u64* __restrict__ edge_of, u32 n, unsigned long long* chosen) {
    u64 took = 0;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const u64 e = best_e[v];
        if (e == MSF_NONE) continue;
        best_e[v] = MSF_NONE;
        if (best_w) best_w[v] = MSF_NONE;
        ++took;
        forest_hook(parent, (u32)(e >> 32), (u32)e, [=](u32 hi) { edge_of[hi] = e; });
    }
    block_add_u64(took, chosen);
}

// the flat forest -> int64 labels (-1 for inactive vertices); cnt[0] += roots among the active vertices; the recorded pairs
// are compacted into rows[] / cols[] (any order), cnt[1] += their number
__global__ __launch_bounds__(256) void msf_finish_kernel(const u32* __restrict__ parent, const u64* __restrict__ act, u32 n,
                                                        const u64* __restrict__ edge_of, long long* __restrict__ out,
                                                        u32* __restrict__ rows, u32* __restrict__ cols,
                                                        unsigned long long* cnt) {
    const u32 lane = lane_id();
    u64 roots = 0;
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 v0 = blockIdx.x * blockDim.x; v0 < n; v0 += stride) {   // (whole waves stay in the loop: the ballot below)
        const u32 v = v0 + threadIdx.x;
        u64 e = MSF_NONE;
        if (v < n) {
            if (vertex_on(act, v)) {
                const u32 r = parent[v];
                out[v] = (long long)r;
                roots += r == v ? 1u : 0u;
                e = edge_of[v];
            } else {
                out[v] = -1;
            }
        }
        const u64 mask = __ballot(e != MSF_NONE);
        if (!mask) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(&cnt[1], (unsigned long long)__builtin_popcountll(mask));
        base = __shfl(base, 0, 64);
        if (e != MSF_NONE) {
            const u64 at = base + wave_slot(mask, lane);
            rows[at] = (u32)(e >> 32);
            cols[at] = (u32)e;
        }
    }
    block_add_u64(roots, &cnt[0]);
}

// value of the stored entry (r, c) of the dense CSR view, or false
__device__ __forceinline__ bool msf_probe(const CsrView& a, const u64* __restrict__ vals, u32 r, u32 c, u64& out) {
    u32 lo = a.rowptr[r], hi = a.rowptr[r + 1];
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (a.colidx[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo >= a.rowptr[r + 1] || a.colidx[lo] != c) return false;
    out = vals[lo];
    return true;
}

// the weight of the forest pair (r, c) for csr_edge_list: the stored value of W(r, c), of W(c, r) when a caller who broke the
// symmetry promise stored only that one; 1.0 for a BOOL W
struct MsfWeight {
    CsrView w;
    const u64* vals;
    __device__ __forceinline__ u64 operator()(u32, u32 r, u32 c) const {
        u64 x = MSF_ONE;
        if (vals && !msf_probe(w, vals, r, c, x)) msf_probe(w, vals, c, r, x);
        return x;
    }
};

struct MsfState {
    const fgpu_mat* W;
    const u64* act;
    u32* parent;
    u64 *done, *rowmin, *chunkmin, *best_w, *best_e;
    uint8_t* cdone;
    unsigned long long* entries;
};

// one scan of the live rows: the word pass + the hub chunks
template <bool VALUED, bool WPASS>
static fgpu_info msf_scan(fgpu_ctx* ctx, const MsfState& s) {
    const fgpu_mat* W = s.W;
    const u32 n = (u32)W->nrows;
    u32 grid = cdiv(cdiv(n, 64), 4);
    if (grid > (u32)ctx->cus * 8) grid = (u32)ctx->cus * 8;
    u64* best = WPASS ? s.best_w : s.best_e;
    FGPU_TRY(launch((msf_rows_kernel<VALUED, WPASS>), dim3(grid), dim3(256), 0, ctx->stream(), view_of(W), (const u64*)W->vals,
                    s.act, (const u32*)s.parent, n, s.done, s.rowmin, (const u64*)s.best_w, best, s.entries));
    if (W->n_hub_chunks)
        FGPU_TRY(launch((msf_hubs_kernel<VALUED, WPASS>), dim3(hub_grid(ctx, W)), dim3(256), 0, ctx->stream(),
                        (const u32*)W->hub_chunks.p, W->n_hub_chunks, (const u32*)W->colidx, (const u64*)W->vals, s.act,
                        (const u32*)s.parent, s.cdone, s.chunkmin, (const u64*)s.best_w, best, s.entries));
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_msf(fgpu_ctx* ctx, const fgpu_mat* W, const uint64_t* active_bitmap, int64_t* component,
                              uint64_t** forest_rows, uint64_t** forest_cols, double** forest_weights, uint64_t* n_forest,
                              uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && W && forest_rows && forest_cols && forest_weights && n_forest, FGPU_NULL_POINTER,
                 "fgpu_msf: NULL argument");
    *forest_rows = *forest_cols = nullptr;
    *forest_weights = nullptr;
    *n_forest = 0;
    FGPU_TRY(check_adjacency("fgpu_msf", W, nullptr));
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)W->nrows;
    if (n == 0) return FGPU_OK;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, W, true));   // (a hypersparse W keeps its values)
    FGPU_TRY(mat_ensure_finalized(W));   // the hub list
    const bool valued = W->vals != nullptr;
    hipStream_t st = ctx->stream();
    const u32 nwords = cdiv(n, 64), nch = W->n_hub_chunks;
    DevBuf<u64> act, done, rowmin, chunkmin, best, edge_of;
    DevBuf<u32> parent, flags, rows, cols;
    DevBuf<uint8_t> cdone;
    DevBuf<unsigned long long> cnt;
    DevBuf<long long> wide;
    if (active_bitmap) FGPU_TRY(upload_active(ctx, act, active_bitmap, n));
    FGPU_TRY(parent.alloc(ctx, n));
    FGPU_TRY(flags.alloc(ctx, FOREST_MAX_JUMPS));
    FGPU_TRY(done.alloc(ctx, nwords));
    FGPU_TRY(best.alloc(ctx, (valued ? 2 : 1) * (size_t)n));   // best_e, best_w
    FGPU_TRY(edge_of.alloc(ctx, n));
    FGPU_TRY(cdone.alloc(ctx, nch));
    if (valued) {
        FGPU_TRY(rowmin.alloc(ctx, n));
        FGPU_TRY(chunkmin.alloc(ctx, nch));
    }
    FGPU_TRY(cnt.alloc(ctx, 4));   // entries read, roots chosen this round, roots, forest pairs
    FGPU_HIP(hipMemsetAsync(done.p, 0, (size_t)nwords * sizeof(u64), st));
    FGPU_HIP(hipMemsetAsync(cdone.p, 0, nch ? nch : 1, st));
    FGPU_HIP(hipMemsetAsync(best.p, 0xFF, (valued ? 2 : 1) * (size_t)n * sizeof(u64), st));
    FGPU_HIP(hipMemsetAsync(edge_of.p, 0xFF, (size_t)n * sizeof(u64), st));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, 4 * sizeof(unsigned long long), st));
    const u32 grid = capped_grid(ctx, n, 256, 4);
    FGPU_TRY(forest_init(ctx, parent.p, n));
    MsfState s;
    s.W = W;
    s.act = act.p;
    s.parent = parent.p;
    s.done = done.p;
    s.rowmin = rowmin.p;
    s.chunkmin = chunkmin.p;
    s.best_e = best.p;
    s.best_w = valued ? best.p + n : nullptr;
    s.cdone = cdone.p;
    s.entries = cnt.p;
    u64 rounds = 0, read_before = 0;
    u32 round_no = 0;
    for (auto& e : ctx->msf_round_entries) e.store(0, std::memory_order_relaxed);
    for (;;) {
        if (valued) {
            FGPU_TRY((msf_scan<true, true>(ctx, s)));
            FGPU_TRY((msf_scan<true, false>(ctx, s)));
        } else {
            FGPU_TRY((msf_scan<false, false>(ctx, s)));
        }
        FGPU_HIP(hipMemsetAsync(cnt.p + 1, 0, sizeof(unsigned long long), st));
        FGPU_TRY(launch(msf_hook_kernel, dim3(grid), dim3(256), 0, st, parent.p, s.best_w, s.best_e, edge_of.p, n, cnt.p + 1));
        u32 w[4];   // entries read so far, roots that chose a pair: one round trip
        FGPU_TRY(read_words(ctx, (const u32*)cnt.p, 4, w));
        const u64 read = (u64)w[0] | ((u64)w[1] << 32), chosen = (u64)w[2] | ((u64)w[3] << 32);
        ctx->msf_round_entries[round_no < 31 ? round_no : 31].fetch_add(read - read_before, std::memory_order_relaxed);
        read_before = read;
        ++round_no;
        if (!chosen) break;   // no component has an external entry
        ++rounds;
        FGPU_TRY(forest_compress(ctx, "fgpu_msf", parent.p, n, flags.p));
    }
    FGPU_TRY(wide.alloc(ctx, n));
    FGPU_TRY(rows.alloc(ctx, n));
    FGPU_TRY(cols.alloc(ctx, n));
    FGPU_TRY(launch(msf_finish_kernel, dim3(grid), dim3(256), 0, st, (const u32*)parent.p, (const u64*)act.p, n,
                    (const u64*)edge_of.p, wide.p, rows.p, cols.p, cnt.p + 2));
    if (component) FGPU_TRY(ctx->d2h(component, wide.p, (size_t)n * sizeof(int64_t)));   // one DMA when component[] is pinned
    unsigned long long h[4];
    FGPU_TRY(ctx->d2h(h, cnt.p, sizeof(h)));
    FGPU_HIP(hipStreamSynchronize(st));
    const u64 k = h[3];
    if (k) {
        // the pairs sorted by (row, col): a CSR of the forest, then the triples
        fgpu_mat* f = nullptr;
        FGPU_TRY(mat_from_device_coo(ctx, &f, n, n, rows.p, cols.p, k));
        FGPU_TRY(csr_edge_list(ctx, "fgpu_msf", "the forest lost pairs in the sort", f, k, MsfWeight{view_of(W), (const u64*)W->vals},
                               4, forest_rows, forest_cols, forest_weights));
        *n_forest = k;
    }
    if (stats) {
        stats[0] = rounds;
        stats[1] = k;
        stats[2] = h[0];
        stats[3] = h[2];
    }
    return FGPU_OK;
}
