// betweenness.hip — algo.betweenness' numeric core: LAGr_Betweenness (called from graph/src/runtime/functions/
// algo_procedures.rs:884-1017 through lagraph_bindings.rs:539-546) over the directed pattern of an adjacency matrix.
//   centrality[v] = sum over the given sources s of delta_s(v),
//   delta_s(v)    = sum over w with v -> w and d_s(w) = d_s(v) + 1 of sigma_s(v) / sigma_s(w) * (1 + delta_s(w)),
// sigma_s the number of shortest directed paths from s, d_s the BFS depth over the out-edges of A.  A source never scores for
// itself (the backward sweep stops at depth 1) and a vertex s does not reach gets nothing from s.
//
// Batched Brandes (the formulation LAGraph publishes): up to 64 sources per batch, source k of the batch is bit k.  Per vertex
// v a u64 frontier word F[v], a next-frontier word N[v] and a visited word V[v]; per (vertex, source) the FP64 path count
// sigma, the FP64 dependency delta and a u32 depth, stored vertex-major with stride B (the batch width) so that the B lanes of
// one lane group read one neighbour's values as one contiguous run.
//
// A lane group is G = pow2ceil(B) consecutive lanes of a wavefront (64 / G groups per wavefront); lane k of a group handles
// source k of the batch.  A group walks one row G entries at a time: lane j loads entry j (column id, and the frontier word /
// depth that decides whether it counts), then the group broadcasts the G entries one by one.
//
// Forward, one depth per step, the host reading three counters per step (read_words: one pinned round trip, ~8 us):
//   push (over A): every frontier row u sends sigma[u][k] to each out-neighbour w whose bit k is not yet visited:
//                  atomicOr(N[w]) + FP64 atomic adds into sigma[w][k] — exact, path counts are integers below 2^53;
//   pull (over At): every vertex with unvisited bits sums sigma[u][k] over its in-neighbours u in the frontier, in row order;
//   rows of HUB_DEG entries and more go through the snapshot's hub chunks in both directions (a workgroup per chunk; the pull
//   chunks of one row meet in FP64 atomic adds, again exact);
//   settle: V |= N, depth of the new bits, the consumed frontier cleared, and the counters of the next step — vertices in the
//   new frontier, out-entries of the new frontier (push cost), in-entries of the vertices with an unvisited bit (pull cost).
//   Direction (bc_direction 0): pull when its cost is below BC_PULL_RATIO x the push cost.
// Backward, depth D-1 down to 1 over A, no atomics: each (v, k) at depth d sums (1 + delta[w][k]) / sigma[w][k] over its
// out-neighbours w at depth d + 1, in row order; delta[v][k] = sigma[v][k] * that sum.  Hub rows: each chunk's partial sum
// (a fixed tree inside the workgroup) into a per-chunk slot, then the chunks of a row summed in chunk order.
// Reduce: centrality[v] += delta[v][k] for k in source order, one thread per vertex; batches run in sequence.
//
// Determinism: sigma is exact whatever order its adds land in, so push, pull and both mixed give identical sigma and depths;
// the backward sums have a fixed order.  Repeated calls and every bc_direction agree bit for bit; batch widths change only
// the grouping inside hub chunks (agreement within rounding).
// Every hand-off between phases is a kernel boundary: nothing reads, inside one launch, a word another workgroup writes in it
// (the kernels that atomically add into sigma[w] / N[w] never read them).  No dynamic LDS; the largest static LDS is the
// reduce buffer of the hub kernels, 2 KiB per workgroup.
#include "algo.hpp"

namespace fgpu {

constexpr u64 BC_PULL_RATIO = 2;            // auto direction: pull when its entries < ratio x the push entries (not tuned)

// the bits of pred over the calling lane's group of 2^lg lanes, lane 0 of the group in bit 0
__device__ __forceinline__ u64 bc_group_ballot(bool pred, u32 lg) {
    const u64 m = __ballot(pred);
    if (lg == 6) return m;
    const u32 base = lane_id() & ~((1u << lg) - 1u);
    return (m >> base) & ((1ull << (1u << lg)) - 1ull);
}

struct BcDev {   // one batch's workspace (device pointers), passed by value
    u64* F;
    u64* N;
    u64* V;
    double* sigma;
    double* delta;
    u32* depth;
    u32 B;       // stride of the per-(vertex, source) arrays = sources in a full batch
    u32 lg;      // log2 of the lane-group size
    u64 full;    // the bits of this batch's sources
};

// the sources of the batch: bit k of N[src[k]], sigma = 1 (a duplicate source is a second bit of the same vertex)
__global__ void bc_seed_kernel(BcDev s, const u64* __restrict__ src, u32 nb) {
    const u32 k = threadIdx.x;
    if (k >= nb) return;
    const u32 v = (u32)src[k];
    atomicOr((unsigned long long*)&s.N[v], (unsigned long long)(1ull << k));
    s.sigma[(size_t)v * s.B + k] = 1.0;
}

// V |= N, depth of the new bits = d1, the consumed frontier F cleared; cnt[0] += vertices of the new frontier, cnt[1] += their
// out-entries in A (the next push), cnt[2] += in-entries of the active vertices that keep an unvisited bit (the next pull)
__global__ __launch_bounds__(256) void bc_settle_kernel(BcDev s, const u32* __restrict__ rpA, const u32* __restrict__ rpAt,
                                                       const u64* __restrict__ act, u32 n, u32 d1, unsigned long long* cnt) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u64 stride = ((u64)gridDim.x * blockDim.x) >> s.lg;
    u64 nf = 0, mf = 0, mu = 0;
    for (u64 vv = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> s.lg; vv < n; vv += stride) {
        const u32 v = (u32)vv;
        const u64 nx = s.N[v];
        if (nx && k < s.B && ((nx >> k) & 1ull)) s.depth[(size_t)v * s.B + k] = d1;
        if (k != 0) continue;
        const u64 vis = s.V[v] | nx;
        if (nx) {
            s.V[v] = vis;
            ++nf;
            mf += rpA[v + 1] - rpA[v];
        }
        s.F[v] = 0;
        if (rpAt && (vis & s.full) != s.full && vertex_on(act, v)) mu += rpAt[v + 1] - rpAt[v];
    }
    block_add_u64(nf, &cnt[0]);
    block_add_u64(mf, &cnt[1]);
    block_add_u64(mu, &cnt[2]);
}

// push, rows shorter than HUB_DEG: a lane group per frontier row u of A
__global__ __launch_bounds__(256) void bc_push_kernel(BcDev s, CsrView a, const u64* __restrict__ act, u32 n) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u64 stride = ((u64)gridDim.x * blockDim.x) >> s.lg;
    for (u64 uu = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> s.lg; uu < n; uu += stride) {
        const u32 u = (u32)uu;
        const u64 fu = s.F[u];
        if (!fu) continue;
        const u32 b = a.rowptr[u], e = a.rowptr[u + 1];
        if (e - b >= HUB_DEG) continue;
        const bool mine = k < s.B && ((fu >> k) & 1ull);
        const double su = mine ? s.sigma[(size_t)u * s.B + k] : 0.0;
        for (u32 base = b; base < e; base += G) {
            u32 wj = 0;
            u64 mj = 0;
            if (base + k < e) {
                wj = a.colidx[base + k];
                if (vertex_on(act, wj)) mj = fu & ~s.V[wj];
            }
            const u32 cnt = e - base < G ? e - base : G;
            for (u32 j = 0; j < cnt; ++j) {
                const u64 m = __shfl(mj, (int)j, (int)G);
                if (!m) continue;
                const u32 w = __shfl(wj, (int)j, (int)G);
                if (k == 0) atomicOr((unsigned long long*)&s.N[w], (unsigned long long)m);
                if (mine && ((m >> k) & 1ull)) unsafeAtomicAdd(&s.sigma[(size_t)w * s.B + k], su);
            }
        }
    }
}

// push, rows of HUB_DEG entries and more: a workgroup per hub chunk of A, its lane groups striding over the chunk
__global__ __launch_bounds__(256) void bc_push_hub_kernel(BcDev s, const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                         const u64* __restrict__ act) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u32 gi = threadIdx.x >> s.lg, ng = 256u >> s.lg;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 u = hub[3 * h], b = hub[3 * h + 1], e = hub[3 * h + 2];
        const u64 fu = s.F[u];
        if (!fu) continue;
        const bool mine = k < s.B && ((fu >> k) & 1ull);
        const double su = mine ? s.sigma[(size_t)u * s.B + k] : 0.0;
        for (u32 base = b + gi * G; base < e; base += ng * G) {
            u32 wj = 0;
            u64 mj = 0;
            if (base + k < e) {
                wj = col[base + k];
                if (vertex_on(act, wj)) mj = fu & ~s.V[wj];
            }
            const u32 cnt = e - base < G ? e - base : G;
            for (u32 j = 0; j < cnt; ++j) {
                const u64 m = __shfl(mj, (int)j, (int)G);
                if (!m) continue;
                const u32 w = __shfl(wj, (int)j, (int)G);
                if (k == 0) atomicOr((unsigned long long*)&s.N[w], (unsigned long long)m);
                if (mine && ((m >> k) & 1ull)) unsafeAtomicAdd(&s.sigma[(size_t)w * s.B + k], su);
            }
        }
    }
}

// pull, rows of At shorter than HUB_DEG: a lane group per active vertex v with an unvisited bit, in-neighbours in row order
__global__ __launch_bounds__(256) void bc_pull_kernel(BcDev s, CsrView at, const u64* __restrict__ act, u32 n) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u64 stride = ((u64)gridDim.x * blockDim.x) >> s.lg;
    for (u64 vv = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> s.lg; vv < n; vv += stride) {
        const u32 v = (u32)vv;
        if (!vertex_on(act, v)) continue;
        const u64 unv = s.full & ~s.V[v];
        if (!unv) continue;
        const u32 b = at.rowptr[v], e = at.rowptr[v + 1];
        if (e - b >= HUB_DEG) continue;
        double acc = 0.0;
        u64 got = 0;
        for (u32 base = b; base < e; base += G) {
            u32 uj = 0;
            u64 fj = 0;
            if (base + k < e) {
                uj = at.colidx[base + k];
                fj = s.F[uj] & unv;
            }
            const u32 cnt = e - base < G ? e - base : G;
            for (u32 j = 0; j < cnt; ++j) {
                const u64 f = __shfl(fj, (int)j, (int)G);
                if (!f) continue;
                const u32 u = __shfl(uj, (int)j, (int)G);
                got |= f;
                if (k < s.B && ((f >> k) & 1ull)) acc += s.sigma[(size_t)u * s.B + k];
            }
        }
        if (!got) continue;
        if (k == 0) s.N[v] = got;
        if (k < s.B && ((got >> k) & 1ull)) s.sigma[(size_t)v * s.B + k] = acc;
    }
}

// pull, rows of At of HUB_DEG entries and more: a workgroup per hub chunk; the lane groups' sums meet in LDS, the chunks of one
// row in FP64 atomic adds (exact: integers)
__global__ __launch_bounds__(256) void bc_pull_hub_kernel(BcDev s, const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                         const u64* __restrict__ act) {
    __shared__ double s_acc[256];
    __shared__ u64 s_got[256];
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u32 gi = threadIdx.x >> s.lg, ng = 256u >> s.lg;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 v = hub[3 * h], b = hub[3 * h + 1], e = hub[3 * h + 2];
        if (!vertex_on(act, v)) continue;
        const u64 unv = s.full & ~s.V[v];   // V does not change during the launch: the same value in every thread
        if (!unv) continue;
        double acc = 0.0;
        u64 got = 0;
        for (u32 base = b + gi * G; base < e; base += ng * G) {
            u32 uj = 0;
            u64 fj = 0;
            if (base + k < e) {
                uj = col[base + k];
                fj = s.F[uj] & unv;
            }
            const u32 cnt = e - base < G ? e - base : G;
            for (u32 j = 0; j < cnt; ++j) {
                const u64 f = __shfl(fj, (int)j, (int)G);
                if (!f) continue;
                const u32 u = __shfl(uj, (int)j, (int)G);
                got |= f;
                if (k < s.B && ((f >> k) & 1ull)) acc += s.sigma[(size_t)u * s.B + k];
            }
        }
        s_acc[threadIdx.x] = acc;
        s_got[threadIdx.x] = got;
        __syncthreads();
        if (threadIdx.x < G) {
            double t = 0.0;
            u64 g = 0;
            for (u32 q = 0; q < ng; ++q) {
                t += s_acc[q * G + threadIdx.x];
                g |= s_got[q * G + threadIdx.x];
            }
            if (threadIdx.x == 0 && g) atomicOr((unsigned long long*)&s.N[v], (unsigned long long)g);
            if (threadIdx.x < s.B && ((g >> threadIdx.x) & 1ull)) unsafeAtomicAdd(&s.sigma[(size_t)v * s.B + threadIdx.x], t);
        }
        __syncthreads();
    }
}

// the sum over v's out-neighbours w at depth d + 1 of (1 + delta[w][k]) / sigma[w][k], entries [b, e) taken G at a time from
// `first` with step `step` (the calling group's share of a hub chunk, or the whole row)
__device__ __forceinline__ double bc_dep_sum(const BcDev& s, const u32* __restrict__ col, u32 first, u32 e, u32 step, u32 k, u32 G,
                                             bool mine, u32 d) {
    double acc = 0.0;
    for (u32 base = first; base < e; base += step) {
        const u32 wj = base + k < e ? col[base + k] : 0u;
        const u32 cnt = e - base < G ? e - base : G;
        for (u32 j = 0; j < cnt; ++j) {
            const u32 w = __shfl(wj, (int)j, (int)G);
            if (!mine) continue;
            const size_t i = (size_t)w * s.B + k;
            if (s.depth[i] == d + 1) acc += (1.0 + s.delta[i]) / s.sigma[i];
        }
    }
    return acc;
}

// backward at depth d, rows of A shorter than HUB_DEG: a lane group per vertex with a source at depth d
__global__ __launch_bounds__(256) void bc_back_kernel(BcDev s, CsrView a, u32 n, u32 d, unsigned long long* entries) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u64 stride = ((u64)gridDim.x * blockDim.x) >> s.lg;
    u64 seen = 0;
    for (u64 vv = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> s.lg; vv < n; vv += stride) {
        const u32 v = (u32)vv;
        const bool mine = k < s.B && s.depth[(size_t)v * s.B + k] == d;
        if (!bc_group_ballot(mine, s.lg)) continue;
        const u32 b = a.rowptr[v], e = a.rowptr[v + 1];
        if (e - b >= HUB_DEG) continue;
        if (k == 0) seen += e - b;
        const double acc = bc_dep_sum(s, a.colidx, b, e, G, k, G, mine, d);
        if (mine) s.delta[(size_t)v * s.B + k] = s.sigma[(size_t)v * s.B + k] * acc;
    }
    block_add_u64(seen, entries);
}

// backward at depth d, hub chunks of A: part[h][k] = the chunk's sum (lane groups strided over the chunk, then a fixed tree)
__global__ __launch_bounds__(256) void bc_back_hub_kernel(BcDev s, const u32* __restrict__ hub, u32 n_hub, const u32* __restrict__ col,
                                                         u32 d, double* __restrict__ part, unsigned long long* entries) {
    __shared__ double s_acc[256];
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u32 gi = threadIdx.x >> s.lg, ng = 256u >> s.lg;
    u64 seen = 0;
    for (u32 h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const u32 v = hub[3 * h], b = hub[3 * h + 1], e = hub[3 * h + 2];
        const bool mine = k < s.B && s.depth[(size_t)v * s.B + k] == d;
        if (!bc_group_ballot(mine, s.lg)) continue;   // the same answer in every group of the workgroup
        if (threadIdx.x == 0) seen += e - b;
        s_acc[threadIdx.x] = bc_dep_sum(s, col, b + gi * G, e, ng * G, k, G, mine, d);
        __syncthreads();
        if (threadIdx.x < G && mine) {
            double t = 0.0;
            for (u32 q = 0; q < ng; ++q) t += s_acc[q * G + threadIdx.x];
            part[(size_t)h * s.B + k] = t;
        }
        __syncthreads();
    }
    block_add_u64(seen, entries);
}

// backward at depth d, hub rows: a lane group per hub chunk that opens a row sums the row's chunks in chunk order (one row's
// chunks are consecutive in the list, mat.hip hub_scan_kernel)
__global__ __launch_bounds__(256) void bc_back_hub_finish_kernel(BcDev s, const u32* __restrict__ hub, u32 n_hub, u32 d,
                                                                const double* __restrict__ part) {
    const u32 G = 1u << s.lg, k = threadIdx.x & (G - 1u);
    const u64 stride = ((u64)gridDim.x * blockDim.x) >> s.lg;
    for (u64 hh = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> s.lg; hh < n_hub; hh += stride) {
        const u32 h = (u32)hh, v = hub[3 * h];
        if (h > 0 && hub[3 * (h - 1)] == v) continue;
        if (k >= s.B || s.depth[(size_t)v * s.B + k] != d) continue;
        double t = 0.0;
        for (u32 q = h; q < n_hub && hub[3 * q] == v; ++q) t += part[(size_t)q * s.B + k];
        s.delta[(size_t)v * s.B + k] = s.sigma[(size_t)v * s.B + k] * t;
    }
}

// centrality[v] += delta[v][k], k in source order
__global__ __launch_bounds__(256) void bc_reduce_kernel(BcDev s, u32 nb, u32 n, double* __restrict__ cent) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const double* dv = s.delta + (size_t)v * s.B;
        double c = cent[v];
        for (u32 k = 0; k < nb; ++k) c += dv[k];
        cent[v] = c;
    }
}

static u32 bc_log2_group(u32 B) {
    u32 lg = 0;
    while ((1u << lg) < B) ++lg;
    return lg;
}

// device bytes of a batch of width B: F, N, V, sigma, delta, depth, plus the hub partial sums
static u64 bc_workspace_bytes(u64 n, u32 B, u32 n_hub) {
    return n * 3 * sizeof(u64) + n * (u64)B * (2 * sizeof(double) + sizeof(u32)) + (u64)n_hub * B * sizeof(double);
}

}  // namespace fgpu

using namespace fgpu;

extern "C" fgpu_info fgpu_betweenness(fgpu_ctx* ctx, const fgpu_mat* A, const fgpu_mat* At, const uint64_t* active_bitmap,
                                      const uint64_t* sources, uint64_t nsrc, double* centrality, uint64_t stats[4]) {
    FGPU_REQUIRE(ctx && A && centrality && (sources || nsrc == 0), FGPU_NULL_POINTER, "fgpu_betweenness: NULL argument");
    FGPU_TRY(check_adjacency("fgpu_betweenness", A, At));
    const u32 n = (u32)A->nrows;
    for (u64 i = 0; i < nsrc; ++i) {
        FGPU_REQUIRE(sources[i] < n, FGPU_OUT_OF_BOUNDS, "fgpu_betweenness: source %llu out of range",
                     (unsigned long long)sources[i]);
        FGPU_REQUIRE(!active_bitmap || ((active_bitmap[sources[i] >> 6] >> (sources[i] & 63)) & 1ull), FGPU_INVALID,
                     "fgpu_betweenness: source %llu is not an active vertex", (unsigned long long)sources[i]);
    }
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (n == 0) return FGPU_OK;
    const int dir = ctx->opt.bc_direction;
    DenseInputs in;
    FGPU_TRY(in.a(ctx, A));
    if (dir == 1) At = nullptr;   // push only: the transpose is never read
    else if (!At) FGPU_TRY(mat_cached_transpose(ctx, A, &At));   // a missing transpose: A's cached one
    FGPU_TRY(in.at(ctx, At));
    FGPU_TRY(mat_ensure_finalized(A));   // the hub lists
    if (At) FGPU_TRY(mat_ensure_finalized(At));
    DevBuf<double> cent;
    FGPU_TRY(cent.alloc(ctx, n));
    FGPU_HIP(hipMemsetAsync(cent.p, 0, (size_t)n * sizeof(double), ctx->stream()));
    u64 st[4] = {0, 0, 0, 0};
    if (nsrc > 0) {
        // batch width: bc_batch, or the smallest of 16 / 32 / 64 that covers nsrc, halved until the workspace fits 3/4 of
        // the free device memory
        u32 B = (u32)ctx->opt.bc_batch;
        if (B == 0) {
            B = nsrc <= 16 ? 16 : nsrc <= 32 ? 32 : 64;
            size_t free_b = 0, total_b = 0;
            FGPU_HIP(hipMemGetInfo(&free_b, &total_b));
            const u64 budget = (u64)free_b / 4 * 3;
            while (B > 1 && bc_workspace_bytes(n, B, A->n_hub_chunks) > budget) B >>= 1;
        }
        DevBuf<u64> act, F, N, V, src;
        DevBuf<double> sigma, delta, part;
        DevBuf<u32> depth;
        DevBuf<unsigned long long> cnt;
        if (active_bitmap) FGPU_TRY(upload_active(ctx, act, active_bitmap, n));
        FGPU_TRY(F.alloc(ctx, n));
        FGPU_TRY(N.alloc(ctx, n));
        FGPU_TRY(V.alloc(ctx, n));
        FGPU_TRY(sigma.alloc(ctx, (size_t)n * B));
        FGPU_TRY(delta.alloc(ctx, (size_t)n * B));
        FGPU_TRY(depth.alloc(ctx, (size_t)n * B));
        FGPU_TRY(part.alloc(ctx, (size_t)(A->n_hub_chunks ? A->n_hub_chunks : 1) * B));
        FGPU_TRY(src.alloc(ctx, nsrc));
        FGPU_TRY(ctx->h2d(src.p, sources, nsrc * sizeof(u64)));
        FGPU_TRY(cnt.alloc(ctx, 4));   // per step: new frontier, push entries, pull entries; [3] backward entries
        FGPU_HIP(hipMemsetAsync(cnt.p, 0, 4 * sizeof(unsigned long long), ctx->stream()));
        BcDev s;
        s.B = B;
        s.lg = bc_log2_group(B);
        const u32 G = 1u << s.lg;
        s.sigma = sigma.p;
        s.delta = delta.p;
        s.depth = depth.p;
        const u64* a = act.p;
        const CsrView va = view_of(A);
        const CsrView vat = At ? view_of(At) : va;
        const u32 ggrid = capped_grid(ctx, (u64)n * G, 256, 16);
        const u32 hgA = hub_grid(ctx, A), hgAt = At ? hub_grid(ctx, At) : 0;
        for (u64 first = 0; first < nsrc; first += B) {
            const u32 nb = (u32)(nsrc - first < B ? nsrc - first : B);
            s.full = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
            s.F = F.p;
            s.N = N.p;
            s.V = V.p;
            FGPU_HIP(hipMemsetAsync(F.p, 0, (size_t)n * sizeof(u64), ctx->stream()));
            FGPU_HIP(hipMemsetAsync(N.p, 0, (size_t)n * sizeof(u64), ctx->stream()));
            FGPU_HIP(hipMemsetAsync(V.p, 0, (size_t)n * sizeof(u64), ctx->stream()));
            FGPU_HIP(hipMemsetAsync(sigma.p, 0, (size_t)n * B * sizeof(double), ctx->stream()));
            FGPU_HIP(hipMemsetAsync(delta.p, 0, (size_t)n * B * sizeof(double), ctx->stream()));
            FGPU_HIP(hipMemsetAsync(depth.p, 0xFF, (size_t)n * B * sizeof(u32), ctx->stream()));   // unreached
            FGPU_TRY(launch(bc_seed_kernel, dim3(1), dim3(64), 0, ctx->stream(), s, (const u64*)src.p + first, nb));
            // forward: settle the frontier of depth d1, read its counters, expand it to depth d1 + 1
            u32 d1 = 0;
            for (;;) {
                FGPU_HIP(hipMemsetAsync(cnt.p, 0, 3 * sizeof(unsigned long long), ctx->stream()));
                FGPU_TRY(launch(bc_settle_kernel, dim3(ggrid), dim3(256), 0, ctx->stream(), s, (const u32*)A->rowptr,
                                At ? (const u32*)At->rowptr : nullptr, a, n, d1, cnt.p));
                std::swap(s.F, s.N);   // the settled frontier is read next; the cleared one collects the next depth
                u32 w[6];
                FGPU_TRY(read_words(ctx, (const u32*)cnt.p, 6, w));
                const u64 nf = w[0] | ((u64)w[1] << 32), mf = w[2] | ((u64)w[3] << 32), mu = w[4] | ((u64)w[5] << 32);
                if (nf == 0) break;
                const bool pull = dir == 2 || (dir == 0 && At && mu < BC_PULL_RATIO * mf);
                if (pull) {
                    FGPU_TRY(launch(bc_pull_kernel, dim3(ggrid), dim3(256), 0, ctx->stream(), s, vat, a, n));
                    if (hgAt) {
                        FGPU_TRY(launch(bc_pull_hub_kernel, dim3(hgAt), dim3(256), 0, ctx->stream(), s,
                                        (const u32*)At->hub_chunks.p, At->n_hub_chunks, (const u32*)At->colidx, a));
                    }
                    st[2] += mu;
                } else {
                    FGPU_TRY(launch(bc_push_kernel, dim3(ggrid), dim3(256), 0, ctx->stream(), s, va, a, n));
                    if (hgA) {
                        FGPU_TRY(launch(bc_push_hub_kernel, dim3(hgA), dim3(256), 0, ctx->stream(), s,
                                        (const u32*)A->hub_chunks.p, A->n_hub_chunks, (const u32*)A->colidx, a));
                    }
                    st[2] += mf;
                }
                ++st[1];
                ++d1;
            }
            const u32 deepest = d1 - 1;   // d1 = the first depth that came out empty
            if (deepest > st[3]) st[3] = deepest;
            ++st[0];
            if (deepest < 2) continue;     // no vertex between a source and a deeper one: every delta is 0
            for (u32 d = deepest - 1; d >= 1; --d) {
                FGPU_TRY(launch(bc_back_kernel, dim3(ggrid), dim3(256), 0, ctx->stream(), s, va, n, d, cnt.p + 3));
                if (hgA) {
                    FGPU_TRY(launch(bc_back_hub_kernel, dim3(hgA), dim3(256), 0, ctx->stream(), s, (const u32*)A->hub_chunks.p,
                                    A->n_hub_chunks, (const u32*)A->colidx, d, part.p, cnt.p + 3));
                    FGPU_TRY(launch(bc_back_hub_finish_kernel, dim3(capped_grid(ctx, (u64)A->n_hub_chunks * G, 256, 16)), dim3(256), 0,
                                    ctx->stream(), s, (const u32*)A->hub_chunks.p, A->n_hub_chunks, d, (const double*)part.p));
                }
            }
            FGPU_TRY(launch(bc_reduce_kernel, dim3(capped_grid(ctx, n, 256, 16)), dim3(256), 0, ctx->stream(), s, nb, n, cent.p));
        }
        u64 back = 0;
        FGPU_TRY(read_u64(ctx, (const u64*)(cnt.p + 3), &back));
        st[2] += back;
    }
    FGPU_TRY(ctx->d2h(centrality, cent.p, (size_t)n * sizeof(double)));   // one DMA when centrality[] is pinned
    if (stats) memcpy(stats, st, sizeof(st));
    FGPU_HIP(hipStreamSynchronize(ctx->stream()));
    return FGPU_OK;
}
