// algo.hpp — the prelude the whole-graph procedures share: each rule below is decided here once.  Included by pagerank.hip,
// wcc.hip, cdlp.hip, harmonic.hip, betweenness.hip, msf.hip, maxflow.hip, by the one-shot fgpu_bfs, and by algo.hip, which holds
// the one copy of the forest's kernels.  What lives here:
//   - the induced subgraph: vertex_on, upload_active; check_adjacency; DenseInputs (hypersparse inputs re-emitted dense);
//   - grids: capped_grid (grid-stride kernels), hub_grid (a workgroup per hub chunk);
//   - wave / workgroup idioms: wave_slot (ballot compaction), block_add_u64 (one atomic per workgroup);
//   - the sort key of a binary64 pattern and its inverse (fp64_sort_key, fp64_from_sort_key);
//   - the union-find forest of fgpu_wcc and fgpu_msf, with its concurrency rules (forest_find, forest_hook, forest_init,
//     forest_compress);
//   - the read-out of a sorted CSR as (row, col, value) result arrays (csr_row_of, csr_edge_list).
// What an algorithm does about a MISSING transpose stays at its call site.
#pragma once
#include "common.hpp"

namespace fgpu {

// is v in the induced subgraph?  (`act` nullable: every vertex is)
__device__ __forceinline__ bool vertex_on(const u64* __restrict__ act, u32 v) {
    return !act || ((act[v >> 6] >> (v & 63)) & 1ull);
}

// the sort key (msf.hip's edge order, fgpu_mat_min_val's minimum) of a stored binary64 pattern: -0.0 is +0.0, then all bits of
// a negative pattern flip and the sign bit of a non-negative one (NaNs sort beyond the infinity of their sign)
__host__ __device__ __forceinline__ u64 fp64_sort_key(u64 b) {
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}
// ... and the pattern of a key (-0.0 comes back as +0.0)
__host__ __device__ __forceinline__ u64 fp64_from_sort_key(u64 k) {
    return (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
}

// ballot compaction: the slot of `lane` among the set lanes of mask = the set lanes below it.  The caller adds the base its
// atomicAdd of popcount(mask) returned (and any stride per lane).
__device__ __forceinline__ u32 wave_slot(u64 mask, u32 lane) {
    return (u32)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
}

// the row r of a dense row-pointer array with rowptr[r] <= i < rowptr[r + 1], i a stored position (nrows > 0)
__device__ __forceinline__ u32 csr_row_of(const u32* __restrict__ rowptr, u32 nrows, u32 i) {
    u32 lo = 0, hi = nrows;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (rowptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// adds a 256-thread workgroup's x into *dst with ONE atomic: one per wave onto a single word serialises (16 K waves of a
// grid-stride launch at RMAT-22 made the count passes 0.26-0.53 ms).  Ends in a barrier: s_part is free again on return,
// so a kernel may call it several times in a row.
__device__ __forceinline__ void block_add_u64(u64 x, unsigned long long* dst) {
    __shared__ u64 s_part[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 t = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (t) atomicAdd(dst, (unsigned long long)t);
    }
    __syncthreads();
}

// The kernels index dense row pointers: a hypersparse input is re-emitted in dense form for the call.  The guard owns those
// temporaries (and a transpose an algorithm builds into dAt itself) and releases them on every exit.
struct DenseInputs {
    MatRef dA, dAt;
    bool densified() const { return dA.get() || dAt.get(); }   // (a temporary stands in for an input: it has no cached indexes or plans)
    // keep_vals: the dense form carries A's UINT64 values (fgpu_msf reads them); the pattern-only algorithms drop them
    fgpu_info a(fgpu_ctx* ctx, const fgpu_mat*& A, bool keep_vals = false) { return dense(ctx, A, dA, keep_vals); }
    fgpu_info at(fgpu_ctx* ctx, const fgpu_mat*& At) { return dense(ctx, At, dAt); }   // NULL stays NULL

   private:
    static fgpu_info dense(fgpu_ctx* ctx, const fgpu_mat*& m, MatRef& own, bool keep_vals = false) {
        if (!m || !m->is_hyper()) return FGPU_OK;
        MatRef prev(std::move(own));   // m itself when the caller built it into this slot: replaced by its dense form
        FGPU_TRY(mat_merge_entries(ctx, &own.m, m, nullptr, nullptr, false, m->nrows, m->ncols, !(keep_vals && m->vals)));
        m = own.get();
        return FGPU_OK;
    }
};

// square; At, if given, of the same dimensions; vertex ids fit u32 with 0xFFFFFFFF left over as "none"
inline fgpu_info check_adjacency(const char* who, const fgpu_mat* A, const fgpu_mat* At) {
    FGPU_REQUIRE(A->nrows == A->ncols, FGPU_DIM_MISMATCH, "%s: adjacency must be square", who);
    FGPU_REQUIRE(!At || (At->nrows == A->nrows && At->ncols == A->ncols), FGPU_DIM_MISMATCH,
                 "%s: transpose has different dimensions", who);
    FGPU_REQUIRE(A->nrows < 0xFFFFFFFFull, FGPU_INVALID, "%s: too many vertices", who);
    return FGPU_OK;
}

// the caller's active bitmap (ceil(n / 64) words, n > 0) on the device, the bits past n — not vertices — cleared in the device
// copy; *count (nullable) = the active vertices
inline fgpu_info upload_active(fgpu_ctx* ctx, DevBuf<u64>& act, const uint64_t* bitmap, u32 n, u64* count = nullptr) {
    const size_t words = ((size_t)n + 63) / 64;
    const u64 last = bitmap[words - 1] & ((n & 63) ? (1ull << (n & 63)) - 1ull : ~0ull);
    FGPU_TRY(act.alloc(ctx, words));
    FGPU_TRY(ctx->h2d(act.p, bitmap, words * sizeof(u64)));
    if (n & 63) FGPU_TRY(ctx->h2d(act.p + words - 1, &last, sizeof(u64)));
    if (count) {
        *count = (u64)__builtin_popcountll(last);
        for (size_t k = 0; k + 1 < words; ++k) *count += (u64)__builtin_popcountll(bitmap[k]);
    }
    return FGPU_OK;
}

// grid of a grid-stride kernel over `items`, `per_block` of them per workgroup and trip: enough workgroups for one trip, at most
// per_cu per CU (a few resident workgroups per CU fill the chip and keep the per-workgroup atomics few), never 0
inline u32 capped_grid(fgpu_ctx* ctx, u64 items, u32 per_block, u32 per_cu) {
    const u64 g = (items + per_block - 1) / per_block, cap = (u64)ctx->cus * per_cu;
    return (u32)(g < 1 ? 1 : (g < cap ? g : cap));
}

// grid of a kernel that strides over m's hub chunks, a workgroup per chunk (0: m has no hub row)
inline u32 hub_grid(fgpu_ctx* ctx, const fgpu_mat* m) {
    const u32 cap = (u32)ctx->cus * 8;
    return m->n_hub_chunks < cap ? m->n_hub_chunks : cap;
}

// ---- the union-find forest (fgpu_wcc, fgpu_msf) ------------------------------------------------------------------------------
// parent[n] over vertex ids; a vertex with parent[v] == v is a root.
// Concurrency rules (inside one launch a plain load can keep returning a word another XCD has since rewritten — per-XCD L2s
// are not coherent; MI355X_MICROARCH.md):
//   - every hook is atomicCAS(&parent[hi], hi, lo) with lo < hi: parent links only point to smaller ids, the forest has no
//     cycles, and a tree's root is its smallest vertex;
//   - a failed CAS continues from the value the CAS RETURNED (fresh, strictly smaller than hi), never from a plain re-load of
//     parent[hi]: the larger of the two roots strictly drops on every retry, so the loop ends within n steps;
//   - the find walk uses plain loads: a stale word is still an ancestor with a smaller id, so the walk ends.  Its path-halving
//     stores write such an ancestor into a word that is already a non-root, which no CAS can succeed on;
//   - a vertex stops being a root once: the thread whose CAS did it is the only one whose forest_hook calls hooked(vertex);
//   - kernel boundaries separate hooking from compression and from whatever reads the flat forest.  Nothing polls or spins on a
//     plain load.
// Compression is pointer jumping by whole launches (parent[v] = parent[parent[v]]) until a launch changes nothing: each halves
// the depth of every tree, so a path of n vertices hooked in id order costs log2(n) launches, not a walk of n per vertex.
constexpr u32 FOREST_MAX_JUMPS = 40;   // pointer-jumping launches of one compress: 33 flatten any forest of < 2^32 vertices

// root of x by plain loads with path halving
__device__ __forceinline__ u32 forest_find(u32* parent, u32 x) {
    for (;;) {
        const u32 p = parent[x];
        if (p == x) return x;
        const u32 gp = parent[p];
        if (gp == p) return p;
        parent[x] = gp;
        x = gp;
    }
}

// join the trees of u and w; hooked(hi) runs once, in the thread whose CAS made the root hi a non-root, and not at all when they
// were one tree already.  (A callback, not a return value: a value returned out of the retry loop reshapes the loop in every
// caller, the ones that drop it included — profiles/NOTES_r13.md section 1.3.)
template <class F>
__device__ __forceinline__ void forest_hook(u32* parent, u32 u, u32 w, F hooked) {
    u32 a = forest_find(parent, u), b = forest_find(parent, w);
    while (a != b) {
        const u32 hi = a > b ? a : b, lo = a > b ? b : a;
        const u32 old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) { hooked(hi); return; }
        a = forest_find(parent, old);   // old < hi: continue from the returned word
        b = forest_find(parent, lo);
    }
}
__device__ __forceinline__ void forest_hook(u32* parent, u32 u, u32 w) {
    forest_hook(parent, u, w, [](u32) {});
}

// algo.hip: parent[v] = v
fgpu_info forest_init(fgpu_ctx* ctx, u32* parent, u32 n);
// algo.hip: pointer jumping until a launch changes nothing, four launches per read-back; flags = FOREST_MAX_JUMPS device words
// of scratch, `who` names the caller in the error text
fgpu_info forest_compress(fgpu_ctx* ctx, const char* who, u32* parent, u32 n, u32* flags);

// ---- a sorted CSR read out as result arrays ------------------------------------------------------------------------------------
// f -> (row, col, value) triples, a thread per stored position i; value(i, row, col) is the triple's 64-bit pattern
template <class V>
__global__ __launch_bounds__(256) void csr_edge_list_kernel(CsrView f, u32 k, V value, u64* __restrict__ orow,
                                                           u64* __restrict__ ocol, u64* __restrict__ oval) {
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        const u32 r = csr_row_of(f.rowptr, f.nrows, i);
        const u32 c = f.colidx[i];
        const u64 x = value(i, r, c);
        orow[i] = r;
        ocol[i] = c;
        oval[i] = x;
    }
}

// Takes over the sorted CSR f (released on every exit) that a COO builder made of k > 0 entries: the triples in (row, col) order
// go out as three result arrays (fgpu_free), which the caller receives only when all three are filled.  `lost` is the error text
// for a builder that merged entries; per_cu caps the grid as capped_grid does.
template <class V>
fgpu_info csr_edge_list(fgpu_ctx* ctx, const char* who, const char* lost, fgpu_mat* f, u64 k, V value, u32 per_cu,
                        uint64_t** rows, uint64_t** cols, double** vals) {
    MatRef own(f);
    FGPU_REQUIRE(f->nnz == k, FGPU_DEVICE, "%s: %s", who, lost);
    DevBuf<u64> trip;
    FGPU_TRY(trip.alloc(ctx, 3 * (size_t)k));
    FGPU_REQUIRE(launch(csr_edge_list_kernel<V>, dim3(capped_grid(ctx, k, 256, per_cu)), dim3(256), 0, ctx->stream(), view_of(f), (u32)k,
                        value, trip.p, trip.p + k, trip.p + 2 * k) == FGPU_OK,
                 FGPU_DEVICE, "%s: launch failed", who);
    ResultBuf out[3];
    for (int j = 0; j < 3; ++j)
        FGPU_REQUIRE(out[j].alloc(ctx, k * sizeof(u64)), FGPU_OOM, "%s: host allocation failed", who);
    for (int j = 0; j < 3; ++j) FGPU_TRY(ctx->d2h(out[j].p, trip.p + j * k, k * sizeof(u64)));
    FGPU_REQUIRE(hipStreamSynchronize(ctx->stream()) == hipSuccess, FGPU_DEVICE, "%s: synchronize failed", who);
    *rows = (uint64_t*)out[0].release();
    *cols = (uint64_t*)out[1].release();
    *vals = (double*)out[2].release();
    return FGPU_OK;
}

}  // namespace fgpu
