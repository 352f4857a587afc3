// algo.hpp — the prelude the whole-graph procedures share (pagerank.hip, wcc.hip, betweenness.hip, msf.hip and the one-shot fgpu_bfs):
// each rule below is decided here once.  Header only; what an algorithm does about a MISSING transpose stays at its call site.
#pragma once
#include "common.hpp"

namespace fgpu {

// is v in the induced subgraph?  (`act` nullable: every vertex is)
__device__ __forceinline__ bool vertex_on(const u64* __restrict__ act, u32 v) {
    return !act || ((act[v >> 6] >> (v & 63)) & 1ull);
}

// the sort key (msf.hip, maxflow.hip's minimum value) of a stored binary64 pattern: -0.0 is +0.0, then all bits of a negative pattern flip and the sign bit of a
// non-negative one (NaNs sort beyond the infinity of their sign)
__host__ __device__ __forceinline__ u64 msf_key(u64 b) {
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
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
    fgpu_mat *dA = nullptr, *dAt = nullptr;
    DenseInputs() {}
    DenseInputs(const DenseInputs&) = delete;
    DenseInputs& operator=(const DenseInputs&) = delete;
    ~DenseInputs() {
        if (dA) mat_release(dA);
        if (dAt) mat_release(dAt);
    }
    bool densified() const { return dA || dAt; }   // (a temporary stands in for an input: it has no cached indexes or plans)
    // keep_vals: the dense form carries A's UINT64 values (fgpu_msf reads them); the pattern-only algorithms drop them
    fgpu_info a(fgpu_ctx* ctx, const fgpu_mat*& A, bool keep_vals = false) { return dense(ctx, A, dA, keep_vals); }
    fgpu_info at(fgpu_ctx* ctx, const fgpu_mat*& At) { return dense(ctx, At, dAt); }   // NULL stays NULL

   private:
    static fgpu_info dense(fgpu_ctx* ctx, const fgpu_mat*& m, fgpu_mat*& own, bool keep_vals = false) {
        if (!m || !m->is_hyper()) return FGPU_OK;
        fgpu_mat* prev = own;   // m itself when the caller built it into this slot: replaced by its dense form
        own = nullptr;
        const fgpu_info i = mat_merge_entries(ctx, &own, m, nullptr, nullptr, false, m->nrows, m->ncols, !(keep_vals && m->vals));
        if (prev) mat_release(prev);
        FGPU_TRY(i);
        m = own;
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

// grid of a kernel that strides over m's hub chunks, a workgroup per chunk (0: m has no hub row)
inline u32 hub_grid(fgpu_ctx* ctx, const fgpu_mat* m) {
    const u32 cap = (u32)ctx->cus * 8;
    return m->n_hub_chunks < cap ? m->n_hub_chunks : cap;
}

}  // namespace fgpu
