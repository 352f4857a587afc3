// edge_layers.hpp — what fgpu_expand_edges (expand_edges.hip) and fgpu_expand_trails (expand_trails.hip) share: fgpu_multi, the
// device view of one relationship tensor's layers (EeType), Tensor::eff_get on it, and the host check that turns the caller's
// per-type layer arrays into that view.  Everything is static or inline: each translation unit carries its own copy.
#pragma once
#include "bulk.hpp"

struct fgpu_multi {
    fgpu_ctx* ctx = nullptr;
    uint64_t n = 0, total = 0;
    fgpu::DevBuf<uint64_t> key, ids;
    fgpu::DevBuf<uint32_t> off;
};

namespace fgpu {

constexpr u64 EE_MAX_ROWS = 1ull << 24;
constexpr int EE_MAX_TYPES = 64;

struct EeType {   // one relationship type; an absent or empty layer is a view of no rows
    CsrView m, dp, dm, tm, tdp, tdm;
    const u64 *mval, *dpval;
    const u64 *mkey, *mids;
    const u32* moff;
    u32 n_multi;
};
// Tensor::eff_get (tensor.rs:286-299): dp's value wins, a dm entry hides m's
__device__ __forceinline__ bool ee_value(const EeType& y, u32 s, u32 d, u64& v) {
    u32 q = probe(y.dp, s, d);
    if (q != ~0u) { v = y.dpval[q]; return true; }
    if (probe(y.dm, s, d) != ~0u) return false;
    q = probe(y.m, s, d);
    if (q == ~0u) return false;
    v = y.mval[q];
    return true;
}
__device__ __forceinline__ bool ee_bit(const u64* __restrict__ bm, u32 v) { return (bm[v >> 6] >> (v & 63)) & 1ull; }
// *total += the sum of x over the wavefront (every lane calls it)
__device__ __forceinline__ void ee_add(u64 x, u64* __restrict__ total) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, WAVE);
    if (lane_id() == 0 && x) atomicAdd((unsigned long long*)total, (unsigned long long)x);
}

static CsrView ee_view(const fgpu_mat* a) {
    if (a && a->nnz) return view_of(a);
    CsrView none;
    none.rowptr = nullptr; none.colidx = nullptr; none.hrows = nullptr; none.nvec = 0; none.nrows = 0;
    return none;
}
static const fgpu_mat* ee_at(const fgpu_mat* const* a, int t) { return a ? a[t] : nullptr; }

// the n_types > 0 tensors of fn as views: every layer n x n with n = m[0]'s dimension < 2^32 - 1, m (and dp) valued
static fgpu_info ee_types(const char* fn, const fgpu_mat* const* m, const fgpu_mat* const* dp, const fgpu_mat* const* dm,
                          const fgpu_mat* const* mt_m, const fgpu_mat* const* mt_dp, const fgpu_mat* const* mt_dm,
                          const fgpu_multi* const* multi, int n_types, std::vector<EeType>& hty, u64& n, bool& any_dp) {
    FGPU_REQUIRE(m[0], FGPU_NULL_POINTER, "%s: m[0] is NULL", fn);
    n = m[0]->nrows;
    FGPU_REQUIRE(n < 0xFFFFFFFFull, FGPU_INVALID, "%s: dimension %llu is past the 32-bit id space", fn, (unsigned long long)n);
    any_dp = false;
    hty.resize((size_t)n_types);
    for (int t = 0; t < n_types; ++t) {
        FGPU_REQUIRE(m[t], FGPU_NULL_POINTER, "%s: m[%d] is NULL", fn, t);
        const fgpu_mat* layer[6] = {m[t], ee_at(dp, t), ee_at(dm, t), ee_at(mt_m, t), ee_at(mt_dp, t), ee_at(mt_dm, t)};
        static const char* const names[6] = {"m", "dp", "dm", "mt_m", "mt_dp", "mt_dm"};
        for (int l = 0; l < 6; ++l)
            FGPU_REQUIRE(!layer[l] || (layer[l]->nrows == n && layer[l]->ncols == n), FGPU_INVALID,
                         "%s: %s[%d] is %llu x %llu, not %llu x %llu", fn, names[l], t, (unsigned long long)layer[l]->nrows,
                         (unsigned long long)layer[l]->ncols, (unsigned long long)n, (unsigned long long)n);
        FGPU_REQUIRE(m[t]->vals || !m[t]->nnz, FGPU_INVALID, "%s: m[%d] must be the tensor's UINT64 base (got a BOOL matrix)", fn, t);
        FGPU_REQUIRE(!layer[1] || !layer[1]->nnz || layer[1]->vals, FGPU_INVALID, "%s: dp[%d] must be UINT64 (got a BOOL matrix)", fn, t);
        EeType& y = hty[t];
        y.m = ee_view(layer[0]); y.dp = ee_view(layer[1]); y.dm = ee_view(layer[2]);
        y.tm = ee_view(layer[3]); y.tdp = ee_view(layer[4]); y.tdm = ee_view(layer[5]);
        y.mval = m[t]->vals;
        y.dpval = layer[1] ? layer[1]->vals : nullptr;
        const fgpu_multi* mu = multi ? multi[t] : nullptr;
        y.mkey = mu ? mu->key.p : nullptr;
        y.mids = mu ? mu->ids.p : nullptr;
        y.moff = mu ? mu->off.p : nullptr;
        y.n_multi = mu ? (u32)mu->n : 0u;
        any_dp = any_dp || y.dp.rowptr || y.tdp.rowptr;
    }
    return FGPU_OK;
}

}  // namespace fgpu
