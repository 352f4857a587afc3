// maxflow.hip — algo.maxFlow's numeric core: LAGr_MaxFlow (called from graph/src/runtime/functions/algo_procedures.rs:3112-3216)
// over a capacity matrix C.  Synchronous push-relabel; the rules (what counts as an arc, what the returned flow must be, when
// the arithmetic is exact) are written out in include/fgpu.h.
//
// Residual network, built once per call: the live arcs of C (off the diagonal, capacity > 0) and their mirrors go through the
// COO builder, so every unordered live pair {u, v} owns the two entries u->v and v->u of a CSR R whose rows come out sorted.
// Per entry a: cap[a] = C(u, v) or 0 (one probe of C), r[a] = the residual (starts at cap[a]), rev[a] = the position of v->u
// (one binary search of row v; R's row pointers are u32, so u32 holds every position).  R is an ordinary snapshot: its hub list
// (rows of HUB_DEG entries and more, cut into chunks) is the one every other algorithm uses.
// State: e[v] (f64) the excess, h[v] (u32) the label; h[src] = n and h[sink] = 0 for ever, neither is ever active.  A vertex is
// active iff e > 0 and h < 2n.  Start: src's arcs are saturated, a global relabel sets h.
// A pulse over the list of active vertices, two kernels (rows below HUB_DEG, a wavefront per listed vertex):
//   push     labels are read-only.  v's budget is the e[v] it loads on entry; over its arcs with r > 0 and h[v] == h[head] + 1,
//            64 at a time, lane k pushes d = min(r, what the budget leaves after the lanes before it) (a wave scan):
//            r[a] -= d by a plain store — two opposite arcs are never both admissible under fixed labels, so v is the only
//            writer of an arc it may push on and nobody pushes on its mirror in this launch — atomicAdd(r[rev[a]], d),
//            atomicAdd(e[head], d), and ONE atomicAdd(e[v], -pushed) at the end.
//   relabel  residuals are read-only.  A listed vertex that pushed nothing sets h[v] = 1 + min h[w] over its arcs with r > 0
//            (2n with none).  Labels only rise: a neighbour relabelling in the same launch reads the old or the new word, the
//            old one is the smaller, and a label computed from a smaller neighbour label is still valid.
// The next list: the atomicAdd on e[head] returns the old word — the thread that saw it go from <= 0 to > 0 appends head; the
// owner appends itself when its own final atomicAdd leaves > 0 (it then also covers "relabelled").  Only the owner lowers e[v]
// and only once, so e[v] crosses zero upwards at most once per launch: a vertex is appended once per pulse.  A pulse reads its
// list's length on the device, appends to the other list and clears the third of three rotating counters; the host reads a
// counter back once per batch of MF_BATCH pulses, the pulses of a batch after the list ran empty return at once.
// Hub rows are not pushed from the list (an entry naming one is skipped).  Their state sits per row in hub-chunk order
// (hfirst[] = a chunk's first chunk of the same row): hub_step (a thread per hub row, after the pulse's other kernels) sets
// bud = e when the row is active.  hub_push, a workgroup per chunk: the chunk's admissible residuals are summed (S), thread 0
// claims take = clamp(atomicAdd(bud, -S)'s old word, 0, S) — the old words fall from e by the S of the chunks before, so the
// takes add up to min(e, sum of S) — and the chunk pushes `take` along its arcs by block scans, then atomicAdd(took, take).
// It never touches e[row]: hub_step applies e -= took in the next phase, so pushes INTO an active hub see e > 0 and the
// crossing rule above holds.  hub_relabel (per chunk, after the push phase) lowers newh by atomicMin for the active hubs that
// took nothing; hub_step applies it, lists the row when it stays active (so the list length still decides termination).
// Global relabel, at the start and then every MF_GLOBAL_EVERY pulses: h = unset, then a level-synchronous backward BFS (a
// wavefront per frontier vertex; v->w's mirror has r > 0 means w reaches v) from sink for h = dist, then from src for
// h = n + dist; a vertex is claimed by atomicCAS(h[w], unset, label), the plain load in front only filters.  What stays unset
// reads as >= 2n.  Levels are batched like pulses.
// Read-out: f(a) = cap[a] - r[a] where positive — of two opposite arcs at most one is — compacted, sorted by the COO builder.
//
// Concurrency rules (per-XCD L2s are not coherent inside a launch; MI355X_MICROARCH.md): inside a launch a word another
// workgroup may write is only touched by device-scope atomics (e[], the mirror residuals, bud / took / newh, the BFS claim of
// h[], list counters); a vertex' own budget is read by an atomic load.  Plain stores go to words with one writer in the launch
// (r[a] of an admissible arc, h[v] of the relabelling owner, list slots handed out by the counter).  Phases are kernel
// boundaries.  Nothing polls or spins.
// No kernel spills; static LDS: 328 bytes (hub_push), none dynamic.
#include "algo.hpp"

namespace fgpu {

constexpr u32 MF_UNSET = 0xFFFFFFFFu;
constexpr u32 MF_BATCH = 16;          // pulses (BFS levels) per read-back of the list length
// pulses between two global relabels (applied at batch boundaries, so a multiple of MF_BATCH).  Swept on the card at RMAT-22
// (profiles/NOTES_r12.md section 6.2): 32 was the fastest, 182 ms; at 8 / 16 the call pays 5-6 relabels of two whole searches each
// (192 / 197 ms), at 64 / 128 the labels go stale and the run needs twice the pulses and pushes (264 / 249 ms), and from 256 on
// the time follows the pulse count (412 ms, 1413 ms at 1024).
constexpr u32 MF_GLOBAL_EVERY = 32;
constexpr u64 MF_CAP_FACTOR = 4;      // hard cap: MF_CAP_FACTOR * (n^2 + n) pulses; the bound of push-relabel is O(n^2) relabels

struct MfNet {
    const u32* rowptr;
    const u32* col;
    const u32* rev;
    double* r;
    double* e;
    u32* h;
    u32 n, src, sink, hmax;
};

__device__ __forceinline__ double mf_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// inclusive wave scan
__device__ __forceinline__ double mf_wave_scan(double x, u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d, 64);
        if (lane >= (u32)d) x += y;
    }
    return x;
}

__device__ __forceinline__ double mf_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// the lanes with `yes` append v to list[] (one atomic per wavefront); every lane of the wavefront calls
__device__ __forceinline__ void mf_append(bool yes, u32 v, u32* __restrict__ list, u32* cnt, u32 lane) {
    const u64 mask = __ballot(yes);
    if (!mask) return;
    u32 base = 0;
    if (lane == 0) base = atomicAdd(cnt, (u32)__builtin_popcountll(mask));
    base = __shfl(base, 0, 64);
    if (yes) list[base + wave_slot(mask, lane)] = v;
}

// one push of d along arc a of the owner (its r[a] is ra); true when the head has to be listed
__device__ __forceinline__ bool mf_push_arc(const MfNet& g, u32 a, u32 w, double ra, double d) {
    g.r[a] = ra - d;
    atomicAdd(&g.r[g.rev[a]], d);
    const double old = atomicAdd(&g.e[w], d);
    return w != g.src && w != g.sink && !(old > 0.0) && old + d > 0.0;
}

// ---- building the residual network ---------------------------------------------------------------------------------------
// live arcs of C and their mirrors as COO pairs (any order); bad += the entries that are NaN or infinite
__global__ __launch_bounds__(256) void mf_arcs_kernel(CsrView c, const u64* __restrict__ vals, u32 nnz, u32* __restrict__ rows,
                                                     u32* __restrict__ cols, unsigned long long* cnt) {
    const u32 lane = lane_id();
    const u32 stride = gridDim.x * blockDim.x;
    u64 bad = 0;
    for (u32 i0 = blockIdx.x * blockDim.x; i0 < nnz; i0 += stride) {   // (whole waves stay in the loop: the ballot below)
        const u32 i = i0 + threadIdx.x;
        bool live = false;
        u32 u = 0, v = 0;
        if (i < nnz) {
            u = csr_row_of(c.rowptr, c.nrows, i);
            v = c.colidx[i];
            double x = 1.0;
            if (vals) {
                const u64 b = vals[i];
                x = __longlong_as_double((long long)b);
                if (((b >> 52) & 0x7FFull) == 0x7FFull) { ++bad; x = 0.0; }
            }
            live = u != v && x > 0.0;
        }
        const u64 mask = __ballot(live);
        if (!mask) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(&cnt[0], 2ull * (u64)__builtin_popcountll(mask));
        base = __shfl(base, 0, 64);
        if (live) {
            const u64 at = base + 2ull * wave_slot(mask, lane);   // (an arc and its mirror)
            rows[at] = u; cols[at] = v;
            rows[at + 1] = v; cols[at + 1] = u;
        }
    }
    block_add_u64(bad, &cnt[1]);
}

// position of column c in row r of the view, or MF_UNSET
__device__ __forceinline__ u32 mf_find(const u32* __restrict__ rowptr, const u32* __restrict__ col, u32 r, u32 c) {
    u32 lo = rowptr[r], hi = rowptr[r + 1];
    const u32 end = hi;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (col[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (lo < end && col[lo] == c) ? lo : MF_UNSET;
}

// a thread per entry of R: its capacity, residual and mirror
__global__ __launch_bounds__(256) void mf_net_kernel(CsrView rv, u32 m, CsrView c, const u64* __restrict__ vals,
                                                    double* __restrict__ cap, double* __restrict__ r, u32* __restrict__ rev) {
    for (u32 a = blockIdx.x * blockDim.x + threadIdx.x; a < m; a += gridDim.x * blockDim.x) {
        const u32 u = csr_row_of(rv.rowptr, rv.nrows, a), v = rv.colidx[a];
        double x = 0.0;
        const u32 at = mf_find(c.rowptr, c.colidx, u, v);
        if (at != MF_UNSET) {
            x = vals ? __longlong_as_double((long long)vals[at]) : 1.0;
            if (!(x > 0.0)) x = 0.0;
        }
        cap[a] = x;
        r[a] = x;
        rev[a] = mf_find(rv.rowptr, rv.colidx, v, u);   // (always there: every pair is stored both ways)
    }
}

// hfirst[k] = the first chunk of chunk k's row
__global__ void mf_hfirst_kernel(const u32* __restrict__ hub, u32 n_hub, u32* __restrict__ hfirst) {
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < n_hub; k += gridDim.x * blockDim.x) {
        u32 f = k;
        while (f > 0 && hub[3 * (f - 1)] == hub[3 * k]) --f;
        hfirst[k] = f;
    }
}

// src's arcs are saturated; the heads are the first active list (one workgroup)
__global__ __launch_bounds__(256) void mf_start_kernel(MfNet g, u32* __restrict__ list, u32* cnt) {
    const u32 lane = lane_id();
    const u32 rb = g.rowptr[g.src], re = g.rowptr[g.src + 1];
    double out = 0.0;
    for (u32 a0 = rb; a0 < re; a0 += 256) {
        const u32 a = a0 + threadIdx.x;
        bool app = false;
        u32 w = 0;
        if (a < re) {
            const double ra = g.r[a];
            w = g.col[a];
            if (ra > 0.0) { app = mf_push_arc(g, a, w, ra, ra); out += ra; }
        }
        mf_append(app, w, list, cnt, lane);
    }
    out = mf_wave_sum(out);
    if (lane == 0 && out > 0.0) atomicAdd(&g.e[g.src], -out);
}

// ---- global relabel --------------------------------------------------------------------------------------------------------
// h[src] = n, h[sink] = 0, the first frontier = {seed}
__global__ void mf_seed_kernel(MfNet g, u32 seed, u32* __restrict__ list, u32* cnt3) {
    g.h[g.src] = g.n;
    g.h[g.sink] = 0;
    list[0] = seed;
    cnt3[0] = 1; cnt3[1] = 0; cnt3[2] = 0;
}

// one level: every vertex w with a residual arc into a frontier vertex and no label yet gets base + level + 1
__global__ __launch_bounds__(256) void mf_bfs_kernel(MfNet g, const u32* __restrict__ cur, u32* __restrict__ next, u32* cnt3,
                                                    u32 level, u32 base) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 count = cnt3[level % 3];
    u32* ncnt = &cnt3[(level + 1) % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt3[(level + 2) % 3] = 0;   // (read last by the level before this one)
    u64 label = (u64)base + level + 1;
    if (label > 0xFFFFFFFEull) label = 0xFFFFFFFEull;
    for (u32 i = wave; i < count; i += nwaves) {
        const u32 v = cur[i];
        const u32 rb = g.rowptr[v], re = g.rowptr[v + 1];
        for (u32 a0 = rb; a0 < re; a0 += 64) {
            const u32 a = a0 + lane;
            bool app = false;
            u32 w = 0;
            if (a < re) {
                w = g.col[a];
                if (g.r[g.rev[a]] > 0.0 && g.h[w] == MF_UNSET) app = atomicCAS(&g.h[w], MF_UNSET, (u32)label) == MF_UNSET;
            }
            mf_append(app, w, next, ncnt, lane);
        }
    }
}

// ---- a pulse -----------------------------------------------------------------------------------------------------------------
// counters: cnt3[] the three rotating list lengths, stat[0] pulses that had work, stat[1] pushes
__global__ __launch_bounds__(256) void mf_push_kernel(MfNet g, const u32* __restrict__ cur, u32* __restrict__ next, u32* cnt3,
                                                     u32 pulse, uint8_t* __restrict__ moved, unsigned long long* stat) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 count = cnt3[pulse % 3];
    u32* ncnt = &cnt3[(pulse + 1) % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt3[(pulse + 2) % 3] = 0;   // (read last by the pulse before this one)
        if (count) atomicAdd(&stat[0], 1ull);
    }
    u64 pushes = 0;
    for (u32 i = wave; i < count; i += nwaves) {
        const u32 v = cur[i];
        const u32 rb = g.rowptr[v], re = g.rowptr[v + 1];
        const u32 hv = g.h[v];
        const double budget = mf_load(&g.e[v]);
        if (re - rb >= HUB_DEG || hv >= g.hmax || !(budget > 0.0)) {   // (wave-uniform) a hub, or not active: nothing to relabel
            if (lane == 0) moved[i] = 1;
            continue;
        }
        double left = budget, pushed = 0.0;
        for (u32 a0 = rb; a0 < re && left > 0.0; a0 += 64) {
            const u32 a = a0 + lane;
            double x = 0.0;
            u32 w = 0;
            if (a < re) {
                w = g.col[a];
                if (g.h[w] + 1u == hv) {
                    const double ra = g.r[a];
                    if (ra > 0.0) x = ra;
                }
            }
            const double inc = mf_wave_scan(x, lane);
            double d = left - (inc - x);
            d = d < x ? d : x;
            bool app = false;
            if (d > 0.0) { app = mf_push_arc(g, a, w, x, d); ++pushes; } else d = 0.0;
            mf_append(app, w, next, ncnt, lane);
            const double tot = mf_wave_sum(d);
            pushed += tot;
            left -= tot;
        }
        bool again = false;
        if (lane == 0) {
            moved[i] = pushed > 0.0 ? 1 : 0;
            again = (pushed > 0.0 ? atomicAdd(&g.e[v], -pushed) - pushed : budget) > 0.0;
        }
        mf_append(again, v, next, ncnt, lane);
    }
    block_add_u64(pushes, &stat[1]);
}

__global__ __launch_bounds__(256) void mf_relabel_kernel(MfNet g, const u32* __restrict__ cur, const u32* cnt3, u32 pulse,
                                                        const uint8_t* __restrict__ moved) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const u32 count = cnt3[pulse % 3];
    for (u32 i = wave; i < count; i += nwaves) {
        if (moved[i]) continue;   // (wave-uniform)
        const u32 v = cur[i];
        const u32 rb = g.rowptr[v], re = g.rowptr[v + 1];
        u32 m = MF_UNSET;
        for (u32 a = rb + lane; a < re; a += 64) {
            if (g.r[a] > 0.0) {
                const u32 hw = g.h[g.col[a]];
                m = hw < m ? hw : m;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u32 y = __shfl_xor(m, d, 64);
            m = y < m ? y : m;
        }
        if (lane == 0) g.h[v] = m < g.hmax ? m + 1u : g.hmax;   // (m + 1 > h[v]: no arc of v was admissible)
    }
}

// ---- hub rows ------------------------------------------------------------------------------------------------------------------
struct MfHub {
    const u32* hub;      // (row, begin, end) per chunk
    const u32* hfirst;
    u32 n_hub;
    double* bud;         // per row, at its first chunk: what the row may still push this pulse (0: not active)
    double* took;        // ... what its chunks pushed
    u32* newh;           // ... 1 + min label over its residual arcs, when it took nothing
};

// inclusive scan of x over the 256 threads; *total = the sum.  Ends in a barrier (s_w is free again).
__device__ __forceinline__ double mf_block_scan(double x, double* s_w, double* total) {
    const u32 lane = lane_id(), wv = threadIdx.x >> 6;
    double inc = mf_wave_scan(x, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    double before = 0.0, tot = 0.0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        if (k < wv) before += s_w[k];
        tot += s_w[k];
    }
    __syncthreads();
    *total = tot;
    return inc + before;
}

__global__ __launch_bounds__(256) void mf_hub_push_kernel(MfNet g, MfHub hb, u32* __restrict__ next, const u32* cnt3, u32 pulse,
                                                         unsigned long long* stat) {
    __shared__ double s_w[4];
    __shared__ double s_take;
    const u32 lane = lane_id();
    u32* ncnt = const_cast<u32*>(&cnt3[(pulse + 1) % 3]);
    u64 pushes = 0;
    for (u32 k = blockIdx.x; k < hb.n_hub; k += gridDim.x) {
        const u32 row = hb.hub[3 * k], b = hb.hub[3 * k + 1], e = hb.hub[3 * k + 2], f = hb.hfirst[k];
        // (thread 0 alone reads the budget word — other chunks lower it meanwhile — so the whole workgroup takes one way)
        if (!__syncthreads_or(threadIdx.x == 0 && mf_load(&hb.bud[f]) > 0.0)) continue;
        const u32 hv = g.h[row];
        double s = 0.0;
        for (u32 a = b + threadIdx.x; a < e; a += 256) {
            if (g.h[g.col[a]] + 1u == hv) {
                const double ra = g.r[a];
                if (ra > 0.0) s += ra;
            }
        }
        double total;
        mf_block_scan(s, s_w, &total);
        if (threadIdx.x == 0) {
            double take = 0.0;
            if (total > 0.0) {
                const double old = atomicAdd(&hb.bud[f], -total);
                take = old < total ? old : total;
                if (!(take > 0.0)) take = 0.0;
            }
            s_take = take;
        }
        __syncthreads();
        double left = s_take;
        __syncthreads();   // s_take is rewritten by the next chunk
        if (!(left > 0.0)) continue;   // (workgroup-uniform)
        double pushed = 0.0;
        for (u32 a0 = b; a0 < e && left > 0.0; a0 += 256) {
            const u32 a = a0 + threadIdx.x;
            double x = 0.0;
            u32 w = 0;
            if (a < e) {
                w = g.col[a];
                if (g.h[w] + 1u == hv) {
                    const double ra = g.r[a];
                    if (ra > 0.0) x = ra;
                }
            }
            double strip;
            const double inc = mf_block_scan(x, s_w, &strip);
            double d = left - (inc - x);
            d = d < x ? d : x;
            bool app = false;
            if (d > 0.0) { app = mf_push_arc(g, a, w, x, d); ++pushes; }
            mf_append(app, w, next, ncnt, lane);
            const double go = strip < left ? strip : left;
            pushed += go;
            left -= go;
        }
        if (threadIdx.x == 0 && pushed > 0.0) atomicAdd(&hb.took[f], pushed);
    }
    block_add_u64(pushes, &stat[1]);
}

__global__ __launch_bounds__(256) void mf_hub_relabel_kernel(MfNet g, MfHub hb) {
    __shared__ u32 s_m[4];
    for (u32 k = blockIdx.x; k < hb.n_hub; k += gridDim.x) {
        const u32 b = hb.hub[3 * k + 1], e = hb.hub[3 * k + 2], f = hb.hfirst[k];
        // bud was set to e > 0 for an active row and only lowered since; took says whether any chunk pushed
        if (hb.newh[f] == 0u || hb.took[f] > 0.0) continue;   // (workgroup-uniform: both words were written by earlier launches)
        u32 m = MF_UNSET;
        for (u32 a = b + threadIdx.x; a < e; a += 256) {
            if (g.r[a] > 0.0) {
                const u32 hw = g.h[g.col[a]];
                m = hw < m ? hw : m;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u32 y = __shfl_xor(m, d, 64);
            m = y < m ? y : m;
        }
        if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int j = 1; j < 4; ++j) m = s_m[j] < m ? s_m[j] : m;
            m = m < g.hmax ? m + 1u : g.hmax;
            atomicMin(&hb.newh[f], m);
        }
        __syncthreads();
    }
}

// a thread per hub row, the last kernel of a pulse: the pulse's pushes leave e, the new label is applied, and the row is
// armed (and listed) for the next pulse when it is active.  newh: 0 = the row was not active in this pulse.
__global__ __launch_bounds__(256) void mf_hub_step_kernel(MfNet g, MfHub hb, u32* __restrict__ next, u32* cnt3, u32 pulse) {
    const u32 lane = lane_id();
    u32* ncnt = &cnt3[(pulse + 1) % 3];
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 k0 = blockIdx.x * blockDim.x; k0 < hb.n_hub; k0 += stride) {   // (whole waves stay in the loop: the ballot in mf_append)
        const u32 k = k0 + threadIdx.x;
        bool on = false;
        u32 row = 0;
        if (k < hb.n_hub && hb.hfirst[k] == k) {
            row = hb.hub[3 * k];
            double ex = g.e[row];
            const u32 nh = hb.newh[k];
            if (nh != 0u) {
                const double t = hb.took[k];
                if (t > 0.0) { ex -= t; g.e[row] = ex; }
                else if (nh != MF_UNSET) g.h[row] = nh;
            }
            on = row != g.src && row != g.sink && ex > 0.0 && g.h[row] < g.hmax;
            hb.bud[k] = on ? ex : 0.0;
            hb.took[k] = 0.0;
            hb.newh[k] = on ? MF_UNSET : 0u;
        }
        mf_append(on, row, next, ncnt, lane);
    }
}

// ---- read-out ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mf_flow_kernel(CsrView rv, u32 m, const double* __restrict__ cap,
                                                     const double* __restrict__ r, const u32* __restrict__ rev,
                                                     u32* __restrict__ rows, u32* __restrict__ cols,
                                                     u64* __restrict__ vals, unsigned long long* cnt) {
    const u32 lane = lane_id();
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 a0 = blockIdx.x * blockDim.x; a0 < m; a0 += stride) {   // (whole waves stay in the loop)
        const u32 a = a0 + threadIdx.x;
        double f = 0.0;
        if (a < m) {
            f = cap[a] - r[a];
            // exact arithmetic makes the mirror's difference -f; capacities whose sums round may leave both a few ulps above
            // zero: the larger one stays
            const u32 b = rev[a];
            const double fb = cap[b] - r[b];
            if (fb > f || (fb == f && b < a)) f = 0.0;
        }
        const bool yes = f > 0.0;
        const u64 mask = __ballot(yes);
        if (!mask) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(cnt, (unsigned long long)__builtin_popcountll(mask));
        base = __shfl(base, 0, 64);
        if (yes) {
            const u64 at = base + wave_slot(mask, lane);
            rows[at] = csr_row_of(rv.rowptr, rv.nrows, a);
            cols[at] = rv.colidx[a];
            vals[at] = (u64)__double_as_longlong(f);
        }
    }
}

// the value of the flow entry at position i for csr_edge_list: the sorted flow CSR's own
struct MfFlowValue {
    const u64* vals;
    __device__ __forceinline__ u64 operator()(u32 i, u32, u32) const { return vals[i]; }
};

// smallest stored value of a valued matrix under fp64_sort_key's order (LAGraph_Cached_EMin): a block reduce, one atomicMin per workgroup
__global__ __launch_bounds__(256) void mf_min_kernel(const u64* __restrict__ vals, u64 nnz, unsigned long long* best) {
    __shared__ u64 s_part[4];
    u64 key = ~0ull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (u64)gridDim.x * blockDim.x) {
        const u64 k = fp64_sort_key(vals[i]);
        key = k < key ? k : key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 y = __shfl_xor(key, d, 64);
        key = y < key ? y : key;
    }
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < 4; ++j) key = s_part[j] < key ? s_part[j] : key;
        atomicMin(best, (unsigned long long)key);
    }
}

struct MfRun {
    fgpu_ctx* ctx;
    MfNet g;
    MfHub hb;
    u32 *list[2], *bfs[2];
    u32 *cnt3, *bcnt3;
    uint8_t* moved;
    unsigned long long* stat;
    u32 grid;       // wave-per-vertex kernels
    u32 hgrid;      // hub chunk kernels (0: no hub row)
};

// one backward BFS: labels base + dist for the unlabelled vertices that reach `seed`
static fgpu_info mf_bfs(MfRun& s, u32 seed, u32 base) {
    hipStream_t st = s.ctx->stream();
    FGPU_TRY(launch(mf_seed_kernel, dim3(1), dim3(1), 0, st, s.g, seed, s.bfs[0], s.bcnt3));
    for (u32 level = 0;;) {
        for (u32 b = 0; b < MF_BATCH; ++b, ++level)
            FGPU_TRY(launch(mf_bfs_kernel, dim3(s.grid), dim3(256), 0, st, s.g, (const u32*)s.bfs[level & 1], s.bfs[(level + 1) & 1],
                            s.bcnt3, level, base));
        u32 left = 0;
        FGPU_TRY(read_u32(s.ctx, s.bcnt3 + level % 3, &left));
        if (!left) return FGPU_OK;
        FGPU_REQUIRE((u64)level <= (u64)s.g.n + MF_BATCH, FGPU_DEVICE, "fgpu_maxflow: a relabel search went past n levels");
    }
}

static fgpu_info mf_global_relabel(MfRun& s) {
    FGPU_HIP(hipMemsetAsync(s.g.h, 0xFF, (size_t)s.g.n * sizeof(u32), s.ctx->stream()));
    FGPU_TRY(mf_bfs(s, s.g.sink, 0));
    return mf_bfs(s, s.g.src, s.g.n);
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_mat_min_val(fgpu_ctx* ctx, const fgpu_mat* A, uint64_t* bits, int* found) {
    FGPU_REQUIRE(ctx && A && bits && found, FGPU_NULL_POINTER, "fgpu_mat_min_val: NULL argument");
    *found = 0;
    *bits = 0;
    if (A->nnz == 0) return FGPU_OK;
    *found = 1;
    if (!A->vals) { *bits = 0x3FF0000000000000ull; return FGPU_OK; }   // BOOL: every value is 1.0
    DevBuf<unsigned long long> best;
    FGPU_TRY(best.alloc(ctx, 1));
    FGPU_HIP(hipMemsetAsync(best.p, 0xFF, sizeof(unsigned long long), ctx->stream()));
    FGPU_TRY(launch(mf_min_kernel, dim3(capped_grid(ctx, A->nnz, 1024, 8)), dim3(256), 0, ctx->stream(), (const u64*)A->vals, A->nnz, best.p));
    u64 key = 0;
    FGPU_TRY(read_u64(ctx, (const u64*)best.p, &key));
    *bits = fp64_from_sort_key(key);   // (-0.0 comes back as +0.0)
    return FGPU_OK;
}

extern "C" fgpu_info fgpu_maxflow(fgpu_ctx* ctx, const fgpu_mat* C, uint64_t src, uint64_t sink, double* max_flow,
                                  uint64_t** flow_rows, uint64_t** flow_cols, double** flow_vals, uint64_t* n_flow,
                                  uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && C && max_flow && flow_rows && flow_cols && flow_vals && n_flow, FGPU_NULL_POINTER,
                 "fgpu_maxflow: NULL argument");
    *flow_rows = *flow_cols = nullptr;
    *flow_vals = nullptr;
    *n_flow = 0;
    *max_flow = 0.0;
    FGPU_TRY(check_adjacency("fgpu_maxflow", C, nullptr));
    FGPU_REQUIRE(src < C->nrows && sink < C->nrows, FGPU_INVALID, "fgpu_maxflow: src / sink out of range");
    FGPU_REQUIRE(src != sink, FGPU_INVALID, "fgpu_maxflow: src == sink");
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const u32 n = (u32)C->nrows;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, C, true));   // (a hypersparse C keeps its values)
    hipStream_t st = ctx->stream();
    DevBuf<unsigned long long> cnt;   // [0] COO pairs, [1] NaN / inf entries, [2] pulses with work, [3] pushes, [4] flow entries
    FGPU_TRY(cnt.alloc(ctx, 5));
    FGPU_HIP(hipMemsetAsync(cnt.p, 0, 5 * sizeof(unsigned long long), st));
    // R holds up to 2 nnz(C) entries at u32 positions, and the grid-stride loops over them step by up to 2^19 in u32: the bound
    // leaves 2^25 of headroom below 2^32, so no counter wraps
    FGPU_REQUIRE(C->nnz < 0x7F000000ull, FGPU_INVALID, "fgpu_maxflow: too many entries for a residual network with 32-bit positions");
    // the residual network
    MatRef net;
    u64 npairs = 0;
    if (C->nnz) {
        DevBuf<u32> rows, cols;
        FGPU_TRY(rows.alloc(ctx, 2 * (size_t)C->nnz));
        FGPU_TRY(cols.alloc(ctx, 2 * (size_t)C->nnz));
        FGPU_TRY(launch(mf_arcs_kernel, dim3(capped_grid(ctx, C->nnz, 256, 8)), dim3(256), 0, st, view_of(C), (const u64*)C->vals,
                        (u32)C->nnz, rows.p, cols.p, cnt.p));
        u32 w[4];
        FGPU_TRY(read_words(ctx, (const u32*)cnt.p, 4, w));
        npairs = (u64)w[0] | ((u64)w[1] << 32);
        FGPU_REQUIRE(!(w[2] | w[3]), FGPU_INVALID, "fgpu_maxflow: a capacity is NaN or infinite");
        if (npairs) FGPU_TRY(mat_from_device_coo(ctx, &net.m, n, n, rows.p, cols.p, npairs));
    }
    const fgpu_mat* R = net.m;
    if (!R || R->nnz == 0) return FGPU_OK;   // no live arc: no flow
    FGPU_TRY(mat_ensure_finalized(R));   // the hub list
    const u32 m = (u32)R->nnz, nch = R->n_hub_chunks;
    DevBuf<double> cap, r, e, bud;
    DevBuf<u32> rev, h, lists, hfirst, newh, cnt3;
    DevBuf<uint8_t> moved;
    FGPU_TRY(cap.alloc(ctx, m));
    FGPU_TRY(r.alloc(ctx, m));
    FGPU_TRY(rev.alloc(ctx, m));
    FGPU_TRY(e.alloc(ctx, n));
    FGPU_TRY(h.alloc(ctx, n));
    const size_t lcap = (size_t)n + nch;   // a vertex is listed once per pulse, a hub row once more by mf_hub_step_kernel
    FGPU_TRY(lists.alloc(ctx, 2 * lcap + 2 * (size_t)n));
    FGPU_TRY(moved.alloc(ctx, lcap));
    FGPU_TRY(cnt3.alloc(ctx, 6));
    FGPU_TRY(bud.alloc(ctx, 2 * (size_t)nch));
    FGPU_TRY(hfirst.alloc(ctx, nch));
    FGPU_TRY(newh.alloc(ctx, nch));
    FGPU_HIP(hipMemsetAsync(e.p, 0, (size_t)n * sizeof(double), st));
    FGPU_HIP(hipMemsetAsync(cnt3.p, 0, 6 * sizeof(u32), st));
    FGPU_HIP(hipMemsetAsync(bud.p, 0, 2 * (size_t)(nch ? nch : 1) * sizeof(double), st));
    FGPU_HIP(hipMemsetAsync(newh.p, 0, (size_t)(nch ? nch : 1) * sizeof(u32), st));
    FGPU_TRY(launch(mf_net_kernel, dim3(capped_grid(ctx, m, 256, 8)), dim3(256), 0, st, view_of(R), m, view_of(C), (const u64*)C->vals,
                    cap.p, r.p, rev.p));
    if (nch) FGPU_TRY(launch(mf_hfirst_kernel, dim3(cdiv(nch, 256)), dim3(256), 0, st, (const u32*)R->hub_chunks.p, nch, hfirst.p));
    MfRun s;
    s.ctx = ctx;
    s.g.rowptr = R->rowptr;
    s.g.col = R->colidx;
    s.g.rev = rev.p;
    s.g.r = r.p;
    s.g.e = e.p;
    s.g.h = h.p;
    s.g.n = n;
    s.g.src = (u32)src;
    s.g.sink = (u32)sink;
    s.g.hmax = 2ull * n < 0xFFFFFFFEull ? 2 * n : 0xFFFFFFFEu;
    s.hb.hub = R->hub_chunks.p;
    s.hb.hfirst = hfirst.p;
    s.hb.n_hub = nch;
    s.hb.bud = bud.p;
    s.hb.took = bud.p + nch;
    s.hb.newh = newh.p;
    s.list[0] = lists.p;
    s.list[1] = lists.p + lcap;
    s.bfs[0] = lists.p + 2 * lcap;
    s.bfs[1] = lists.p + 2 * lcap + n;
    s.cnt3 = cnt3.p;
    s.bcnt3 = cnt3.p + 3;
    s.moved = moved.p;
    s.stat = cnt.p + 2;
    s.grid = capped_grid(ctx, n, 4, 8);
    s.hgrid = nch ? hub_grid(ctx, R) : 0;
    const u32 sgrid = nch ? capped_grid(ctx, nch, 256, 8) : 0;
    // start: src's arcs saturated into list 0 (the length lands in cnt3[0]), labels by a global relabel, the hub rows armed
    FGPU_TRY(launch(mf_start_kernel, dim3(1), dim3(256), 0, st, s.g, s.list[0], s.cnt3));
    FGPU_TRY(mf_global_relabel(s));
    u64 relabels = 1;
    int64_t every = MF_GLOBAL_EVERY;
    if (ctx->opt.maxflow_global_every > 0) every = ctx->opt.maxflow_global_every;
    const u64 nn = (u64)n * n + n;
    const u64 cap_pulses = nn > ~0ull / MF_CAP_FACTOR ? ~0ull : MF_CAP_FACTOR * nn;
    u64 pulse = 0;
    if (nch) {
        // (pulse "-1": lists into list[0] behind what the start left there)
        FGPU_TRY(launch(mf_hub_step_kernel, dim3(sgrid), dim3(256), 0, st, s.g, s.hb, s.list[0], s.cnt3, 2u));
    }
    for (;;) {
        for (u32 b = 0; b < MF_BATCH; ++b, ++pulse) {
            const u32 p = (u32)(pulse % 6);   // (the list parity and the counter rotation repeat every 6 pulses)
            u32* cur = s.list[p & 1];
            u32* next = s.list[(p + 1) & 1];
            FGPU_TRY(launch(mf_push_kernel, dim3(s.grid), dim3(256), 0, st, s.g, (const u32*)cur, next, s.cnt3, p, s.moved, s.stat));
            if (nch) FGPU_TRY(launch(mf_hub_push_kernel, dim3(s.hgrid), dim3(256), 0, st, s.g, s.hb, next, (const u32*)s.cnt3, p, s.stat));
            FGPU_TRY(launch(mf_relabel_kernel, dim3(s.grid), dim3(256), 0, st, s.g, (const u32*)cur, (const u32*)s.cnt3, p,
                            (const uint8_t*)s.moved));
            if (nch) {
                FGPU_TRY(launch(mf_hub_relabel_kernel, dim3(s.hgrid), dim3(256), 0, st, s.g, s.hb));
                FGPU_TRY(launch(mf_hub_step_kernel, dim3(sgrid), dim3(256), 0, st, s.g, s.hb, next, s.cnt3, p));
            }
        }
        u32 left = 0;
        FGPU_TRY(read_u32(ctx, s.cnt3 + (pulse % 6) % 3, &left));
        if (!left) break;
        FGPU_REQUIRE(pulse < cap_pulses, FGPU_INVALID, "fgpu_maxflow: no flow after %llu pulses (the cap for %u vertices)",
                     (unsigned long long)pulse, n);
        if (pulse / (u64)every >= relabels) {
            FGPU_TRY(mf_global_relabel(s));
            ++relabels;
        }
    }
    // read-out
    DevBuf<u32> frows, fcols;
    DevBuf<u64> fvals;
    FGPU_TRY(frows.alloc(ctx, m / 2));   // (of two opposite arcs at most one carries flow)
    FGPU_TRY(fcols.alloc(ctx, m / 2));
    FGPU_TRY(fvals.alloc(ctx, m / 2));
    FGPU_TRY(launch(mf_flow_kernel, dim3(capped_grid(ctx, m, 256, 8)), dim3(256), 0, st, view_of(R), m, (const double*)cap.p,
                    (const double*)r.p, (const u32*)rev.p, frows.p, fcols.p, fvals.p, cnt.p + 4));
    unsigned long long hc[5];
    double value = 0.0;
    FGPU_TRY(ctx->d2h(hc, cnt.p, sizeof(hc)));
    FGPU_TRY(ctx->d2h(&value, e.p + sink, sizeof(double)));
    FGPU_HIP(hipStreamSynchronize(st));
    const u64 k = hc[4];
    if (k) {
        fgpu_mat* f = nullptr;
        FGPU_TRY(mat_from_device_coo_vals(ctx, &f, n, n, frows.p, fcols.p, fvals.p, k));
        FGPU_TRY(csr_edge_list(ctx, "fgpu_maxflow", "the flow lost entries in the sort", f, k, MfFlowValue{(const u64*)f->vals}, 8,
                               flow_rows, flow_cols, flow_vals));
        *n_flow = k;
    }
    *max_flow = value;
    if (stats) {
        stats[0] = hc[2];
        stats[1] = relabels;
        stats[2] = m;
        stats[3] = hc[3];
    }
    return FGPU_OK;
}
