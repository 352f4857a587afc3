// sssp.hip — algo.SPpaths' numeric core: the single-source shortest-path problem behind the reference's dijkstra_single_path
// (graph/src/runtime/functions/algo_procedures.rs:2156-2257; no LAGraph call stands behind it).  Near / far delta-stepping
// for the distances, then a level-synchronous search over the tight entries for the parents; the rules (what a weight may be,
// which distance and which parent come back) are written out in include/fgpu.h.
// fgpu_sssp_hops, the hop-bounded table that prunes the procedure's enumeration shapes, is the second half of the file; it shares
// the weight pass, sp_weight and the row kernel's entry-parallel layout.
//
// Phase 1, distances.  dist[] holds binary64 bit patterns: non-negative finite doubles order as unsigned integers and
// 0x7FF0... is "unreached".  T is the upper edge of the current bucket, a multiple of the width delta (a power of two).
//   near pile   (vertex, distance) pairs below T, two lists that swap every step;
//   far pile    vertices at or beyond T, one entry per vertex (infar[] is the membership flag), two lists that swap per split.
// A step is four launches that take every decision on the device (SsspCtl), so the host queues steps blindly:
//   rows     64 entries of the current near list per wavefront.  An entry whose stored distance is no longer dist[u] is
//            stale and dropped (lazy deletion).  The out-entries of the live rows below HUB_DEG are relaxed entry-parallel
//            over the 64 rows (columns and values coalesced along each row); a live row of HUB_DEG and more is stamped in
//            hubmark[] for the next kernel.
//   hubs     a workgroup per hub chunk of the snapshot; the chunks of a stamped row relax from the dist[row] of this launch.
//   control  one thread: the lists swap; when the near pile ran empty and the far pile did not, T moves to the end of the
//            bucket that holds the far pile's minimum (empty buckets are skipped; a T that no longer separates, delta below
//            the spacing of the doubles at that distance, becomes +inf: everything is near) and a split is ordered.
//   split    the far list: an entry below the previous T was served from the near pile already and leaves, one below T
//            moves to the near pile, the rest is kept and its minimum recomputed.
// A relaxation lowers dist[v] with ONE 64-bit atomicMin; the lane whose atomic lowered the word appends v (ballot
// compaction, one atomicAdd per wavefront and pile).  Sizes: a launch reads every live row once, so it appends at most nnz near
// entries; a vertex is in the far list once.  The appends are bounds-checked all the same (SsspCtl::overflow).
// The host reads {done, overflow} back once per SSSP_BATCH steps.
//
// Phase 2, parents (skipped when neither parent nor stats is wanted).  An entry (u, v), u != v, is tight when dist[u] + w is
// finite and equals dist[v].  A wavefront per frontier vertex pushes over its tight entries: u32 atomicMin of level + 1 into
// depth[v]; the lane that found it unset appends v.  In a level-synchronous search every u with depth[u] + 1 == depth[v] meets
// v in the same launch, where the word the atomic returned is "unset" or level + 1: exactly those lanes lower par[v] with a
// u32 atomicMin of u — the smallest qualifying u, with no further pass over the entries.
//
// Concurrency rules (per-XCD L2s are not coherent inside a launch; MI355X_MICROARCH.md):
//   - dist[], depth[], par[] are only ever lowered by atomicMin inside a launch; the plain load in front of the atomic is a
//     filter: a stale word is a LARGER one, so a skipped atomic would have changed nothing;
//   - a row is relaxed from the dist[u] a plain load returns at the pop: the words were written by earlier launches.  Should
//     another lane lower dist[u] in this launch, it also appends u again;
//   - hubmark[], infar[] (cleared by the split), the control block and the list slots handed out by a counter have one writer
//     per launch or are touched by atomics only.  Phases are kernel boundaries.  Nothing polls or spins.
// No kernel spills; static LDS: 5.0 KiB (rows kernel); no dynamic LDS.
#include "algo.hpp"

#include <math.h>

namespace fgpu {

constexpr u64 SP_INF = 0x7FF0000000000000ull;    // +inf: "unreached", and the T that takes everything
constexpr u64 SP_ONE = 0x3FF0000000000000ull;    // 1.0
constexpr u64 SP_NEG0 = 0x8000000000000000ull;
constexpr u32 SP_UNSET = 0xFFFFFFFFu;
constexpr u32 SSSP_BATCH = 4;         // steps (levels of phase 2) per read-back of the control block
constexpr u64 SSSP_CAP_FACTOR = 4;    // hard cap: SSSP_CAP_FACTOR * (n^2 + n) + 64 steps

// the device-side control block; the host reads the first two words
struct SsspCtl {
    u32 done, overflow;
    u32 np, fp;            // which near list is the current one, which far list takes the appends
    u32 ncnt[2], fcnt[2];  // list lengths
    u32 split;             // the split kernel of this step has work
    u32 pad;
    u64 T, Tprev, farmin;
    double delta;
    unsigned long long launches, popped, entries;   // stats[0..2]
    unsigned long long bad, nfinite;                // the weight pass
    double wsum;
    u32 lcnt[3];           // phase 2: rotating frontier lengths
    u32 maxdepth;
};

struct SsspLists {
    u32* nearv[2];
    u64* neard[2];
    u32* farv[2];
    u32 ncap, fcap;
};

__device__ __forceinline__ u64 sp_weight(const u64* __restrict__ vals, u32 i) {
    if (!vals) return SP_ONE;
    const u64 b = vals[i];
    return b == SP_NEG0 ? 0ull : b;
}

// the two steps of the entry-parallel layout both rows kernels use: 64 rows per wavefront, their lengths summed along the
// lanes, then a lane per ENTRY that finds its row in the LDS copy of the sums
__device__ __forceinline__ u32 wave_inclusive_sum(u32 x, u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d, 64);
        if (lane >= (u32)d) x += y;
    }
    return x;
}
// off[0 .. 64]: the exclusive prefix of the 64 rows' lengths; the largest row with off[row] <= e
__device__ __forceinline__ u32 row_of_entry(const u32* off, u32 e) {
    u32 lo = 0, hi = 64;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const u32 mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// one pass over the values: NaNs and negative weights are counted, the finite ones summed (the mean behind delta)
__global__ __launch_bounds__(256) void sssp_weights_kernel(const u64* __restrict__ vals, u64 nnz, SsspCtl* ctl) {
    __shared__ double s_sum[4];
    u64 bad = 0, fin = 0;
    double sum = 0.0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (u64)gridDim.x * blockDim.x) {
        const u64 b = vals[i];
        if (b == SP_NEG0) { ++fin; continue; }
        if ((b >> 63) || b > SP_INF) { ++bad; continue; }   // a sign bit, or a NaN
        if (b < SP_INF) { ++fin; sum += __longlong_as_double((long long)b); }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane_id() == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (t > 0.0) atomicAdd(&ctl->wsum, t);
    }
    block_add_u64(bad, &ctl->bad);
    block_add_u64(fin, &ctl->nfinite);
}

__global__ __launch_bounds__(256) void sssp_init_kernel(u64* __restrict__ dist, u32* __restrict__ infar, u32* __restrict__ hubmark,
                                                       u32 n) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        dist[v] = SP_INF;
        infar[v] = 0;
        hubmark[v] = 0;
    }
}

// one thread: delta (log2 forced by the caller, or from the mean finite weight and the mean degree), the first bucket, the source
__global__ void sssp_start_kernel(SsspCtl* ctl, SsspLists ls, u64* __restrict__ dist, u32 src, u64 nnz, u32 n, int valued,
                                  int forced, int log2_forced) {
    double delta;
    if (forced) {
        delta = ldexp(1.0, log2_forced);
    } else if (!valued) {
        delta = 1.0;   // every weight is 1.0: a bucket is a BFS level
    } else {
        // 32 relaxations' worth of mean weight per mean row (the near / far heuristic of Davidson et al., IPDPS 2014), as a power of two
        const double meanw = ctl->nfinite ? ctl->wsum / (double)ctl->nfinite : 0.0;
        const double deg = nnz > n ? (double)nnz / (double)n : 1.0;
        const double want = 32.0 * meanw / deg;
        if (want > 0.0 && want < __longlong_as_double((long long)SP_INF)) {
            int e;
            frexp(want, &e);
            delta = ldexp(1.0, e);
        } else {
            delta = __longlong_as_double((long long)SP_INF);   // all weights zero (or their sum overflowed): one bucket
        }
    }
    if (!(delta > 0.0)) delta = 4.9406564584124654e-324;   // (ldexp below the subnormals)
    ctl->delta = delta;
    ctl->T = (u64)__double_as_longlong(delta);
    ctl->Tprev = 0;
    ctl->farmin = SP_INF;
    dist[src] = 0;
    ls.nearv[0][0] = src;
    ls.neard[0][0] = 0;
    ctl->ncnt[0] = 1;
}

// the lanes whose atomic lowered dist[c] to nd file c: below T in the next near list, the others in the far list (once per vertex)
__device__ __forceinline__ void sssp_file(bool won, u32 c, u64 nd, u64 T, SsspCtl* ctl, const SsspLists& ls, u32 nnext, u32 fcur,
                                          u32* __restrict__ infar, u32 lane) {
    const bool nearw = won && nd < T;
    const u64 nmask = __ballot(nearw);
    if (nmask) {
        u32 base = 0;
        if (lane == 0) base = atomicAdd(&ctl->ncnt[nnext], (u32)__builtin_popcountll(nmask));
        base = __shfl(base, 0, 64);
        if (nearw) {
            const u64 at = (u64)base + wave_slot(nmask, lane);
            if (at < ls.ncap) { ls.nearv[nnext][at] = c; ls.neard[nnext][at] = nd; }
            else ctl->overflow = 1;
        }
    }
    const bool farw = won && nd >= T;
    if (__ballot(farw)) {
        u64 m = farw ? nd : SP_INF;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 y = __shfl_xor(m, d, 64);
            m = y < m ? y : m;
        }
        if (lane == 0 && ctl->farmin > m) atomicMin((unsigned long long*)&ctl->farmin, (unsigned long long)m);
        const bool fresh = farw && atomicExch(&infar[c], 1u) == 0u;
        const u64 fmask = __ballot(fresh);
        if (fmask) {
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&ctl->fcnt[fcur], (u32)__builtin_popcountll(fmask));
            base = __shfl(base, 0, 64);
            if (fresh) {
                const u64 at = (u64)base + wave_slot(fmask, lane);
                if (at < ls.fcap) ls.farv[fcur][at] = c;
                else ctl->overflow = 1;
            }
        }
    }
}

// relaxes the entry at position idx of row u (distance du); every lane of the wavefront calls, `valid` or not
__device__ __forceinline__ void sssp_relax(bool valid, u32 u, u64 du, u32 idx, const u32* __restrict__ col,
                                           const u64* __restrict__ vals, u64* dist, u64 T, SsspCtl* ctl, const SsspLists& ls,
                                           u32 nnext, u32 fcur, u32* __restrict__ infar, u32 lane) {
    bool won = false;
    u32 c = 0;
    u64 nd = SP_INF;
    if (valid) {
        c = col[idx];
        const double s = __longlong_as_double((long long)du) + __longlong_as_double((long long)sp_weight(vals, idx));
        nd = (u64)__double_as_longlong(s);
        // (a sum that is not finite is skipped; the diagonal could never lower its own row)
        if (c != u && nd < SP_INF && dist[c] > nd) won = atomicMin((unsigned long long*)&dist[c], (unsigned long long)nd) > nd;
    }
    sssp_file(won, c, nd, T, ctl, ls, nnext, fcur, infar, lane);
}

__global__ __launch_bounds__(256) void sssp_rows_kernel(CsrView a, const u64* __restrict__ vals, u64* dist, SsspCtl* ctl,
                                                       SsspLists ls, u32* __restrict__ infar, u32* __restrict__ hubmark,
                                                       u32 stamp) {
    __shared__ u32 s_off[4][65];   // exclusive prefix of the 64 rows' taken lengths
    __shared__ u32 s_rb[4][64];    // first entry of each row
    __shared__ u32 s_u[4][64];     // the row
    __shared__ u64 s_du[4][64];    // its distance
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 cur = ctl->np, nnext = cur ^ 1u, fcur = ctl->fp;
    const u32 count = ctl->ncnt[cur];
    const u64 T = ctl->T;
    const u32* __restrict__ curv = ls.nearv[cur];
    const u64* __restrict__ curd = ls.neard[cur];
    u32* off = s_off[wv];
    u32* rbs = s_rb[wv];
    u32* us = s_u[wv];
    u64* dus = s_du[wv];
    u64 popped = 0, seen = 0;
    const u32 ngroups = (count + 63) >> 6;
    for (u32 g = wave; g < ngroups; g += nwaves) {
        const u32 i = (g << 6) + lane;
        u32 u = 0, rb = 0, len = 0;
        u64 du = 0;
        if (i < count) {
            u = curv[i];
            du = curd[i];
            if (dist[u] == du) {   // else stale: a later entry of u carries the lower distance
                ++popped;
                rb = a.rowptr[u];
                len = a.rowptr[u + 1] - rb;
                if (len >= HUB_DEG) { hubmark[u] = stamp; len = 0; }
            }
        }
        const u32 inc = wave_inclusive_sum(len, lane);
        const u32 total = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        if (!total) continue;   // (wave-uniform)
        __builtin_amdgcn_wave_barrier();   // (the lanes of the trip before are done with the arrays)
        off[lane + 1] = inc;
        if (lane == 0) off[0] = 0;
        rbs[lane] = rb;
        us[lane] = u;
        dus[lane] = du;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) seen += total;
        for (u32 e0 = 0; e0 < total; e0 += 64) {
            const u32 e = e0 + lane;
            const bool valid = e < total;
            const u32 lo = row_of_entry(off, e);
            const u32 idx = valid ? rbs[lo] + (e - off[lo]) : 0u;
            sssp_relax(valid, us[lo], dus[lo], idx, a.colidx, vals, dist, T, ctl, ls, nnext, fcur, infar, lane);
        }
    }
    block_add_u64(popped, &ctl->popped);
    block_add_u64(seen, &ctl->entries);
}

// the rows of HUB_DEG entries and more: a workgroup per chunk of the snapshot's hub list, for the rows stamped in this step
__global__ __launch_bounds__(256) void sssp_hubs_kernel(const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                       const u64* __restrict__ vals, u64* dist, SsspCtl* ctl, SsspLists ls,
                                                       u32* __restrict__ infar, const u32* __restrict__ hubmark, u32 stamp) {
    const u32 lane = lane_id();
    const u32 nnext = ctl->np ^ 1u, fcur = ctl->fp;
    const u64 T = ctl->T;
    u64 seen = 0;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 row = hub[3 * h], b = hub[3 * h + 1], e = hub[3 * h + 2];
        if (hubmark[row] != stamp) continue;   // (workgroup-uniform: written by the launch before)
        const u64 du = dist[row];
        for (u32 i0 = b; i0 < e; i0 += 256) {   // (whole waves stay in the loop: the ballots of sssp_file)
            const u32 i = i0 + threadIdx.x;
            sssp_relax(i < e, row, du, i < e ? i : b, col, vals, dist, T, ctl, ls, nnext, fcur, infar, lane);
        }
        if (threadIdx.x == 0) seen += e - b;
    }
    if (threadIdx.x == 0 && seen) atomicAdd(&ctl->entries, (unsigned long long)seen);
}

// one thread, after the relaxations of a step: swaps the near lists and orders a split when the bucket is finished
__global__ void sssp_control_kernel(SsspCtl* ctl) {
    const u32 cur = ctl->np;
    if (ctl->ncnt[cur]) ++ctl->launches;
    const u32 np = cur ^ 1u;
    ctl->np = np;
    ctl->ncnt[cur] = 0;   // the list just read is the next one to fill
    ctl->split = 0;
    if (ctl->ncnt[np]) return;
    const u32 fp = ctl->fp;
    if (!ctl->fcnt[fp]) { ctl->done = 1; return; }
    // the bucket of the far pile's minimum: T = (floor(farmin / delta) + 1) * delta, exact for a power of two until it overflows
    const double fm = __longlong_as_double((long long)ctl->farmin), delta = ctl->delta;
    double t = (floor(fm / delta) + 1.0) * delta;
    u64 T = (u64)__double_as_longlong(t);
    if (!(t > fm) || T > SP_INF) T = SP_INF;   // delta is below the spacing of the doubles there (or fm / delta overflowed)
    ctl->Tprev = ctl->T;
    ctl->T = T;
    ctl->farmin = SP_INF;
    ctl->fp = fp ^ 1u;
    ctl->fcnt[fp ^ 1u] = 0;
    ctl->split = 1;
}

__global__ __launch_bounds__(256) void sssp_split_kernel(const u64* __restrict__ dist, SsspCtl* ctl, SsspLists ls,
                                                        u32* __restrict__ infar) {
    if (!ctl->split) return;
    const u32 lane = lane_id();
    const u32 np = ctl->np, fp = ctl->fp, from = fp ^ 1u;
    const u32 count = ctl->fcnt[from];
    const u64 T = ctl->T, Tprev = ctl->Tprev;
    const u32* __restrict__ src = ls.farv[from];
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 i0 = blockIdx.x * blockDim.x; i0 < count; i0 += stride) {   // (whole waves stay in the loop: the ballots below)
        const u32 i = i0 + threadIdx.x;
        bool tonear = false, keep = false;
        u32 v = 0;
        u64 d = SP_INF;
        if (i < count) {
            v = src[i];
            d = dist[v];
            if (d < Tprev) infar[v] = 0;   // lowered into an earlier bucket since: the near pile served it
            else if (d < T) { infar[v] = 0; tonear = true; }
            else keep = true;
        }
        const u64 nmask = __ballot(tonear);
        if (nmask) {
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&ctl->ncnt[np], (u32)__builtin_popcountll(nmask));
            base = __shfl(base, 0, 64);
            if (tonear) {
                const u64 at = (u64)base + wave_slot(nmask, lane);
                if (at < ls.ncap) { ls.nearv[np][at] = v; ls.neard[np][at] = d; }
                else ctl->overflow = 1;
            }
        }
        const u64 kmask = __ballot(keep);
        if (kmask) {
            u64 m = keep ? d : SP_INF;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const u64 y = __shfl_xor(m, s, 64);
                m = y < m ? y : m;
            }
            u32 base = 0;
            if (lane == 0) {
                if (ctl->farmin > m) atomicMin((unsigned long long*)&ctl->farmin, (unsigned long long)m);
                base = atomicAdd(&ctl->fcnt[fp], (u32)__builtin_popcountll(kmask));
            }
            base = __shfl(base, 0, 64);
            if (keep) {
                const u64 at = (u64)base + wave_slot(kmask, lane);
                if (at < ls.fcap) ls.farv[fp][at] = v;
                else ctl->overflow = 1;
            }
        }
    }
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------------------
__global__ void sssp_seed_kernel(SsspCtl* ctl, u32* __restrict__ depth, u32* __restrict__ par, u32* __restrict__ list, u32 src) {
    depth[src] = 0;
    par[src] = src;
    list[0] = src;
    ctl->lcnt[0] = 1; ctl->lcnt[1] = 0; ctl->lcnt[2] = 0;
    ctl->maxdepth = 0;
}

// one level: a wavefront per frontier vertex over its tight entries
__global__ __launch_bounds__(256) void sssp_tight_kernel(CsrView a, const u64* __restrict__ vals, const u64* __restrict__ dist,
                                                        u32* depth, u32* par, const u32* __restrict__ cur, u32* __restrict__ next,
                                                        u32 ncap, SsspCtl* ctl, u32 level) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 count = ctl->lcnt[level % 3];
    u32* ncnt = &ctl->lcnt[(level + 1) % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->lcnt[(level + 2) % 3] = 0;   // (read last by the level before this one)
        if (count) ctl->maxdepth = level;
    }
    u64 seen = 0;
    for (u32 i = wave; i < count; i += nwaves) {
        const u32 u = cur[i];
        const u32 rb = a.rowptr[u], re = a.rowptr[u + 1];
        const double du = __longlong_as_double((long long)dist[u]);
        if (lane == 0) seen += re - rb;
        for (u32 k0 = rb; k0 < re; k0 += 64) {
            const u32 k = k0 + lane;
            bool app = false;
            u32 v = 0;
            if (k < re) {
                v = a.colidx[k];
                const u64 s = (u64)__double_as_longlong(du + __longlong_as_double((long long)sp_weight(vals, k)));
                if (v != u && s < SP_INF && s == dist[v] && depth[v] > level) {
                    const u32 old = atomicMin(&depth[v], level + 1u);
                    app = old == SP_UNSET;
                    if (old > level && par[v] > u) atomicMin(&par[v], u);   // (old is "unset" or level + 1)
                }
            }
            const u64 mask = __ballot(app);
            if (!mask) continue;
            u32 base = 0;
            if (lane == 0) base = atomicAdd(ncnt, (u32)__builtin_popcountll(mask));
            base = __shfl(base, 0, 64);
            if (app) {
                const u64 at = (u64)base + wave_slot(mask, lane);
                if (at < ncap) next[at] = v;
                else ctl->overflow = 1;
            }
        }
    }
    block_add_u64(seen, &ctl->entries);
}

// par[] (u32, "unset" = none) -> the caller's int64 parents
__global__ __launch_bounds__(256) void sssp_parent_kernel(const u32* __restrict__ par, u32 n, long long* __restrict__ out) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        out[v] = par[v] == SP_UNSET ? -1ll : (long long)par[v];
}

// ---- fgpu_sssp_hops: the hop-bounded table ---------------------------------------------------------------------------------------
// D_h = the cheapest route of at most h arcs, one row of the table per h (the rules: include/fgpu.h).  Round h is four launches
// that take every decision on the device (HopsCtl), so the host queues max_hops rounds blindly and reads back once:
//   copy     D_h = D_{h-1}, every vertex.  A round relaxes INTO D_h and reads only D_{h-1}: one round never travels two arcs;
//   rows     the frontier (the vertices round h-1 lowered; a vertex that did not change contributed its D_{h-1} already, so
//            pushing from the changed ones alone is exact), 64 of it per wavefront, rows below HUB_DEG relaxed entry-parallel
//            as sssp_rows_kernel does, longer rows stamped in hubmark[] with the round;
//   hubs     a workgroup per hub chunk of a row stamped this round;
//   control  one thread: the two frontier lists swap, the first round that lowered nothing is recorded.
// Once the frontier is empty the copy alone runs: the remaining rows repeat the last live one.
// Concurrency rules, beyond those of phase 1 above:
//   - D_{h-1} is read-only in round h (plain loads of words earlier launches wrote); D_h is written by the copy launch, then
//     only lowered by atomicMin in the rows and hubs launches, behind a plain-load filter (a stale word is a larger one);
//   - a lane whose atomic lowered D_h[v] claims v for the next frontier with atomicExch(&seen[v], h): the one lane that did not
//     get h back appends, so a vertex is in a frontier once per round and a list of n slots cannot overflow (checked all the same);
//   - hubmark[] has one value per launch (h), the control block one writer (the control launch) or atomics.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): hops_init 8 VGPRs, hops_start 2, hops_copy 6, hops_rows 42
// VGPRs and 5168 B static LDS, hops_hubs 18, hops_control 4; no other LDS, no kernel spills (SGPR or VGPR), no scratch.
struct HopsCtl {
    u32 overflow;
    u32 cur;        // which list is this round's frontier
    u32 cnt[2];     // list lengths
    u32 fixed;      // the first round that lowered nothing, 0 = none yet
    u32 pad;
    unsigned long long rounds, popped, entries;   // stats[0..2]
};

__global__ __launch_bounds__(256) void hops_init_kernel(u64* __restrict__ d0, u32* __restrict__ seen, u32* __restrict__ hubmark,
                                                       u32 n) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        d0[v] = SP_INF;
        seen[v] = 0;
        hubmark[v] = 0;
    }
}

__global__ void hops_start_kernel(HopsCtl* ctl, u64* __restrict__ d0, u32* __restrict__ list0, u32 src) {
    d0[src] = 0;
    list0[0] = src;
    ctl->cnt[0] = 1;
}

__global__ __launch_bounds__(256) void hops_copy_kernel(const u64* __restrict__ prev, u64* __restrict__ cur, u32 n) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) cur[v] = prev[v];
}

// relaxes the entry at position idx of row u (du = D_{h-1}[u]) into dcur = D_h; every lane of the wavefront calls, `valid` or not
__device__ __forceinline__ void hops_relax(bool valid, u32 u, u64 du, u32 idx, const u32* __restrict__ col,
                                           const u64* __restrict__ vals, u64* dcur, u32* seen, u32 h, HopsCtl* ctl,
                                           u32* ncnt, u32* __restrict__ next, u32 cap, u32 lane) {
    bool fresh = false;
    u32 c = 0;
    if (valid) {
        c = col[idx];
        const double s = __longlong_as_double((long long)du) + __longlong_as_double((long long)sp_weight(vals, idx));
        const u64 nd = (u64)__double_as_longlong(s);
        if (c != u && nd < SP_INF && dcur[c] > nd && atomicMin((unsigned long long*)&dcur[c], (unsigned long long)nd) > nd)
            fresh = atomicExch(&seen[c], h) != h;
    }
    const u64 mask = __ballot(fresh);
    if (!mask) return;
    u32 base = 0;
    if (lane == 0) base = atomicAdd(ncnt, (u32)__builtin_popcountll(mask));
    base = __shfl(base, 0, 64);
    if (fresh) {
        const u64 at = (u64)base + wave_slot(mask, lane);
        if (at < cap) next[at] = c;
        else ctl->overflow = 1;
    }
}

__global__ __launch_bounds__(256) void hops_rows_kernel(CsrView a, const u64* __restrict__ vals, const u64* __restrict__ dprev,
                                                       u64* dcur, HopsCtl* ctl, u32* list0, u32* list1, u32 cap, u32* seen,
                                                       u32* __restrict__ hubmark, u32 h) {
    __shared__ u32 s_off[4][65];   // exclusive prefix of the 64 rows' taken lengths
    __shared__ u32 s_rb[4][64];    // first entry of each row
    __shared__ u32 s_u[4][64];     // the row
    __shared__ u64 s_du[4][64];    // its D_{h-1}
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 cur = ctl->cur;
    const u32 count = ctl->cnt[cur];
    const u32* __restrict__ curv = cur ? list1 : list0;
    u32* next = cur ? list0 : list1;
    u32* ncnt = &ctl->cnt[cur ^ 1u];
    u32* off = s_off[wv];
    u32* rbs = s_rb[wv];
    u32* us = s_u[wv];
    u64* dus = s_du[wv];
    u64 popped = 0, read = 0;
    const u32 ngroups = (count + 63) >> 6;
    for (u32 g = wave; g < ngroups; g += nwaves) {
        const u32 i = (g << 6) + lane;
        u32 u = 0, rb = 0, len = 0;
        u64 du = 0;
        if (i < count) {
            u = curv[i];
            du = dprev[u];
            ++popped;
            rb = a.rowptr[u];
            len = a.rowptr[u + 1] - rb;
            if (len >= HUB_DEG) { hubmark[u] = h; len = 0; }
        }
        const u32 inc = wave_inclusive_sum(len, lane);
        const u32 total = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        if (!total) continue;   // (wave-uniform)
        __builtin_amdgcn_wave_barrier();   // (the lanes of the trip before are done with the arrays)
        off[lane + 1] = inc;
        if (lane == 0) off[0] = 0;
        rbs[lane] = rb;
        us[lane] = u;
        dus[lane] = du;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) read += total;
        for (u32 e0 = 0; e0 < total; e0 += 64) {
            const u32 e = e0 + lane;
            const bool valid = e < total;
            const u32 lo = row_of_entry(off, e);
            const u32 idx = valid ? rbs[lo] + (e - off[lo]) : 0u;
            hops_relax(valid, us[lo], dus[lo], idx, a.colidx, vals, dcur, seen, h, ctl, ncnt, next, cap, lane);
        }
    }
    block_add_u64(popped, &ctl->popped);
    block_add_u64(read, &ctl->entries);
}

// the rows of HUB_DEG entries and more: a workgroup per chunk of the snapshot's hub list, for the rows stamped in this round
__global__ __launch_bounds__(256) void hops_hubs_kernel(const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                       const u64* __restrict__ vals, const u64* __restrict__ dprev, u64* dcur,
                                                       HopsCtl* ctl, u32* list0, u32* list1, u32 cap, u32* seen,
                                                       const u32* __restrict__ hubmark, u32 h) {
    const u32 lane = lane_id();
    const u32 cur = ctl->cur;
    u32* next = cur ? list0 : list1;
    u32* ncnt = &ctl->cnt[cur ^ 1u];
    u64 read = 0;
    for (u32 k = blockIdx.x; k < n_hub; k += gridDim.x) {
        const u32 row = hub[3 * k], b = hub[3 * k + 1], e = hub[3 * k + 2];
        if (hubmark[row] != h) continue;   // (workgroup-uniform: written by the launch before)
        const u64 du = dprev[row];
        for (u32 i0 = b; i0 < e; i0 += 256) {   // (whole waves stay in the loop: the ballot of hops_relax)
            const u32 i = i0 + threadIdx.x;
            hops_relax(i < e, row, du, i < e ? i : b, col, vals, dcur, seen, h, ctl, ncnt, next, cap, lane);
        }
        if (threadIdx.x == 0) read += e - b;
    }
    if (threadIdx.x == 0 && read) atomicAdd(&ctl->entries, (unsigned long long)read);
}

// one thread, after the relaxations of round h
__global__ void hops_control_kernel(HopsCtl* ctl, u32 h) {
    const u32 cur = ctl->cur, nxt = cur ^ 1u;
    if (ctl->cnt[cur]) ++ctl->rounds;
    if (!ctl->cnt[nxt] && !ctl->fixed) ctl->fixed = h;   // nothing was lowered: D_h == D_{h-1}
    ctl->cnt[cur] = 0;   // the list just read is the next one to fill
    ctl->cur = nxt;
}

// the one reduction pass over W's values in front of either search: a NaN or a negative weight is FGPU_INVALID
static fgpu_info sssp_check_weights(fgpu_ctx* ctx, const char* who, const fgpu_mat* W, SsspCtl* ctl) {
    const u64* vals = (const u64*)W->vals;
    if (!vals || !W->nnz) return FGPU_OK;
    FGPU_TRY(launch(sssp_weights_kernel, dim3(capped_grid(ctx, W->nnz, 1024, 8)), dim3(256), 0, ctx->stream(), vals, W->nnz, ctl));
    u32 w[2];
    FGPU_TRY(read_words(ctx, (const u32*)&ctl->bad, 2, w));
    FGPU_REQUIRE(!(w[0] | w[1]), FGPU_INVALID, "%s: a weight is NaN or negative", who);
    return FGPU_OK;
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_sssp_hops(fgpu_ctx* ctx, const fgpu_mat* W, uint64_t src, int32_t max_hops, double* table,
                                    uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && W && table, FGPU_NULL_POINTER, "fgpu_sssp_hops: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_sssp_hops", W, nullptr));
    FGPU_REQUIRE(max_hops >= 0 && max_hops <= FGPU_SSSP_HOPS_MAX, FGPU_INVALID, "fgpu_sssp_hops: max_hops must be 0 .. %d, not %d",
                 FGPU_SSSP_HOPS_MAX, (int)max_hops);
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)W->nrows;
    if (n == 0) return FGPU_OK;
    FGPU_REQUIRE(src < W->nrows, FGPU_OUT_OF_BOUNDS, "fgpu_sssp_hops: src out of range");
    DenseInputs in;
    FGPU_TRY(in.a(ctx, W, true));   // (a hypersparse W keeps its values)
    FGPU_TRY(mat_ensure_finalized(W));   // the hub list
    hipStream_t st = ctx->stream();
    const u32 nch = W->n_hub_chunks;
    const u64* vals = (const u64*)W->vals;
    {
        DevBuf<SsspCtl> wctl;
        FGPU_TRY(wctl.alloc(ctx, 1));
        FGPU_HIP(hipMemsetAsync(wctl.p, 0, sizeof(SsspCtl), st));
        FGPU_TRY(sssp_check_weights(ctx, "fgpu_sssp_hops", W, wctl.p));
    }
    const u32 H = (u32)max_hops;
    DevBuf<HopsCtl> ctl;
    DevBuf<u64> tab;
    DevBuf<u32> list, seen, hubmark;
    FGPU_TRY(ctl.alloc(ctx, 1));
    FGPU_TRY(tab.alloc(ctx, ((size_t)H + 1) * n));
    FGPU_TRY(list.alloc(ctx, 2 * (size_t)n));   // a vertex is in a frontier once per round
    FGPU_TRY(seen.alloc(ctx, n));
    FGPU_TRY(hubmark.alloc(ctx, n));
    FGPU_HIP(hipMemsetAsync(ctl.p, 0, sizeof(HopsCtl), st));
    const u32 vgrid = capped_grid(ctx, n, 256, 4), rgrid = capped_grid(ctx, n, 256, 8);
    FGPU_TRY(launch(hops_init_kernel, dim3(vgrid), dim3(256), 0, st, tab.p, seen.p, hubmark.p, n));
    FGPU_TRY(launch(hops_start_kernel, dim3(1), dim3(1), 0, st, ctl.p, tab.p, list.p, (u32)src));
    for (u32 h = 1; h <= H; ++h) {   // (h is never 0, what seen[] and hubmark[] start as)
        const u64* dprev = tab.p + (size_t)(h - 1) * n;
        u64* dcur = tab.p + (size_t)h * n;
        FGPU_TRY(launch(hops_copy_kernel, dim3(vgrid), dim3(256), 0, st, dprev, dcur, n));
        FGPU_TRY(launch(hops_rows_kernel, dim3(rgrid), dim3(256), 0, st, view_of(W), vals, dprev, dcur, ctl.p, list.p, list.p + n, n,
                        seen.p, hubmark.p, h));
        if (nch)
            FGPU_TRY(launch(hops_hubs_kernel, dim3(hub_grid(ctx, W)), dim3(256), 0, st, (const u32*)W->hub_chunks.p, nch,
                            (const u32*)W->colidx, vals, dprev, dcur, ctl.p, list.p, list.p + n, n, seen.p,
                            (const u32*)hubmark.p, h));
        FGPU_TRY(launch(hops_control_kernel, dim3(1), dim3(1), 0, st, ctl.p, h));
    }
    HopsCtl hc;
    FGPU_TRY(ctx->d2h(&hc, ctl.p, sizeof(HopsCtl)));
    FGPU_REQUIRE(!hc.overflow, FGPU_DEVICE, "fgpu_sssp_hops: a frontier outgrew its bound");
    FGPU_TRY(ctx->d2h(table, tab.p, ((size_t)H + 1) * n * sizeof(double)));   // one DMA when table[] is pinned
    if (stats) {
        stats[0] = hc.rounds;
        stats[1] = hc.popped;
        stats[2] = hc.entries;
        stats[3] = hc.fixed ? hc.fixed : H + 1;
    }
    FGPU_HIP(hipStreamSynchronize(st));
    return FGPU_OK;
}

extern "C" fgpu_info fgpu_sssp(fgpu_ctx* ctx, const fgpu_mat* W, uint64_t src, double* dist, int64_t* parent, uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && W && dist, FGPU_NULL_POINTER, "fgpu_sssp: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_sssp", W, nullptr));
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)W->nrows;
    if (n == 0) return FGPU_OK;
    FGPU_REQUIRE(src < W->nrows, FGPU_OUT_OF_BOUNDS, "fgpu_sssp: src out of range");
    DenseInputs in;
    FGPU_TRY(in.a(ctx, W, true));   // (a hypersparse W keeps its values)
    FGPU_TRY(mat_ensure_finalized(W));   // the hub list
    hipStream_t st = ctx->stream();
    const u64 nnz = W->nnz;
    const u32 nch = W->n_hub_chunks;
    const u64* vals = (const u64*)W->vals;
    DevBuf<SsspCtl> ctl;
    FGPU_TRY(ctl.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(ctl.p, 0, sizeof(SsspCtl), st));
    FGPU_TRY(sssp_check_weights(ctx, "fgpu_sssp", W, ctl.p));
    // a launch appends at most one near entry per entry it reads, a split at most n; a vertex is in the far list once
    const u64 ncap64 = (nnz > n ? nnz : (u64)n) + 1;
    FGPU_REQUIRE(ncap64 < 0xFFFFFFFFull, FGPU_INVALID, "fgpu_sssp: too many entries");
    DevBuf<u64> d, neard;
    DevBuf<u32> nearv, farv, infar, hubmark;
    FGPU_TRY(d.alloc(ctx, n));
    FGPU_TRY(neard.alloc(ctx, 2 * (size_t)ncap64));
    FGPU_TRY(nearv.alloc(ctx, 2 * (size_t)ncap64));
    FGPU_TRY(farv.alloc(ctx, 2 * (size_t)n));
    FGPU_TRY(infar.alloc(ctx, n));
    FGPU_TRY(hubmark.alloc(ctx, n));
    SsspLists ls;
    ls.ncap = (u32)ncap64;
    ls.fcap = n;
    for (int k = 0; k < 2; ++k) {
        ls.nearv[k] = nearv.p + (size_t)k * ncap64;
        ls.neard[k] = neard.p + (size_t)k * ncap64;
        ls.farv[k] = farv.p + (size_t)k * n;
    }
    const u32 vgrid = capped_grid(ctx, n, 256, 4);
    FGPU_TRY(launch(sssp_init_kernel, dim3(vgrid), dim3(256), 0, st, d.p, infar.p, hubmark.p, n));
    const int forced = ctx->opt.sssp_delta_log2 != SSSP_DELTA_AUTO;
    FGPU_TRY(launch(sssp_start_kernel, dim3(1), dim3(1), 0, st, ctl.p, ls, d.p, (u32)src, nnz, n, vals ? 1 : 0, forced,
                    forced ? ctx->opt.sssp_delta_log2 : 0));
    const u32 rgrid = capped_grid(ctx, n, 256, 8);
    const u64 nn = (u64)n * n + n;
    const u64 cap_steps = nn > (~0ull - 64) / SSSP_CAP_FACTOR ? ~0ull : SSSP_CAP_FACTOR * nn + 64;
    for (u64 step = 0;;) {
        for (u32 b = 0; b < SSSP_BATCH; ++b, ++step) {
            const u32 stamp = (u32)(step % 0xFFFFFFFEull) + 1u;   // never 0, what hubmark[] starts as
            FGPU_TRY(launch(sssp_rows_kernel, dim3(rgrid), dim3(256), 0, st, view_of(W), vals, d.p, ctl.p, ls, infar.p, hubmark.p, stamp));
            if (nch)
                FGPU_TRY(launch(sssp_hubs_kernel, dim3(hub_grid(ctx, W)), dim3(256), 0, st, (const u32*)W->hub_chunks.p, nch,
                                (const u32*)W->colidx, vals, d.p, ctl.p, ls, infar.p, (const u32*)hubmark.p, stamp));
            FGPU_TRY(launch(sssp_control_kernel, dim3(1), dim3(1), 0, st, ctl.p));
            FGPU_TRY(launch(sssp_split_kernel, dim3(vgrid), dim3(256), 0, st, (const u64*)d.p, ctl.p, ls, infar.p));
        }
        u32 w[2];   // done, overflow: one round trip per batch; the steps queued behind the last one found nothing to do
        FGPU_TRY(read_words(ctx, (const u32*)ctl.p, 2, w));
        FGPU_REQUIRE(!w[1], FGPU_DEVICE, "fgpu_sssp: a worklist outgrew its bound");
        if (w[0]) break;
        FGPU_REQUIRE(step < cap_steps, FGPU_INVALID, "fgpu_sssp: no fixed point after %llu steps (the cap for %u vertices)",
                     (unsigned long long)step, n);
    }
    FGPU_TRY(ctx->d2h(dist, d.p, (size_t)n * sizeof(double)));   // one DMA when dist[] is pinned
    if (parent || stats) {
        DevBuf<u32> depth, par;
        FGPU_TRY(depth.alloc(ctx, n));
        FGPU_TRY(par.alloc(ctx, n));
        FGPU_HIP(hipMemsetAsync(depth.p, 0xFF, (size_t)n * sizeof(u32), st));
        FGPU_HIP(hipMemsetAsync(par.p, 0xFF, (size_t)n * sizeof(u32), st));
        u32* fl[2] = {nearv.p, nearv.p + ncap64};   // the frontier lists: a vertex is appended once, n <= the near capacity
        FGPU_TRY(launch(sssp_seed_kernel, dim3(1), dim3(1), 0, st, ctl.p, depth.p, par.p, fl[0], (u32)src));
        const u32 wgrid = capped_grid(ctx, n, 4, 8);
        for (u32 level = 0;;) {
            for (u32 b = 0; b < SSSP_BATCH; ++b, ++level)
                FGPU_TRY(launch(sssp_tight_kernel, dim3(wgrid), dim3(256), 0, st, view_of(W), vals, (const u64*)d.p, depth.p, par.p,
                                (const u32*)fl[level & 1], fl[(level + 1) & 1], n, ctl.p, level));
            u32 left = 0, over = 0;
            FGPU_TRY(read_u32(ctx, &ctl.p->lcnt[level % 3], &left));
            if (!left) break;
            FGPU_TRY(read_u32(ctx, &ctl.p->overflow, &over));
            FGPU_REQUIRE(!over, FGPU_DEVICE, "fgpu_sssp: a frontier outgrew its bound");
            FGPU_REQUIRE((u64)level <= (u64)n + SSSP_BATCH, FGPU_DEVICE, "fgpu_sssp: the parent search went past n levels");
        }
        if (parent) {
            DevBuf<long long> wide;
            FGPU_TRY(wide.alloc(ctx, n));
            FGPU_TRY(launch(sssp_parent_kernel, dim3(vgrid), dim3(256), 0, st, (const u32*)par.p, n, wide.p));
            FGPU_TRY(ctx->d2h(parent, wide.p, (size_t)n * sizeof(int64_t)));
        }
    }
    SsspCtl h;
    FGPU_TRY(ctx->d2h(&h, ctl.p, sizeof(SsspCtl)));
    ctx->sssp_last_delta.store(h.delta < HUGE_VAL ? (int64_t)ilogb(h.delta) : 1024, std::memory_order_relaxed);
    if (stats) {
        stats[0] = h.launches;
        stats[1] = h.popped;
        stats[2] = h.entries;
        stats[3] = h.maxdepth;
    }
    FGPU_HIP(hipStreamSynchronize(st));
    return FGPU_OK;
}
