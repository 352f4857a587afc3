// algo.hip — the kernels of the prelude that exist once: the union-find forest's initialisation and compression (fgpu_wcc,
// fgpu_msf).  The rules they run under are written out in algo.hpp.
#include "algo.hpp"

namespace fgpu {

__global__ void forest_init_kernel(u32* __restrict__ parent, u32 n) {
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) parent[v] = v;
}

// one pointer-jumping step; flags[k] = 1 when it changed a word.  A launch after one that changed nothing returns at once.
// (No hooks run here: a vertex whose parent's parent is its parent points at a root.)
__global__ __launch_bounds__(256) void forest_jump_kernel(u32* parent, u32 n, u32* flags, u32 k) {
    if (k > 0 && flags[k - 1] == 0) return;
    bool changed = false;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const u32 p = parent[v];
        const u32 gp = parent[p];
        if (gp != p) { parent[v] = gp; changed = true; }
    }
    if (__ballot(changed) != 0ull && lane_id() == 0) flags[k] = 1u;
}

// (grid-stride: 1 K workgroups of 256 fill the chip)
fgpu_info forest_init(fgpu_ctx* ctx, u32* parent, u32 n) {
    FGPU_TRY(launch(forest_init_kernel, dim3(capped_grid(ctx, n, 256, 4)), dim3(256), 0, ctx->stream(), parent, n));
    return FGPU_OK;
}

fgpu_info forest_compress(fgpu_ctx* ctx, const char* who, u32* parent, u32 n, u32* flags) {
    constexpr u32 BATCH = 4;   // launches per read-back
    FGPU_HIP(hipMemsetAsync(flags, 0, FOREST_MAX_JUMPS * sizeof(u32), ctx->stream()));
    const u32 grid = capped_grid(ctx, n, 256, 4);
    for (u32 k = 0; k < FOREST_MAX_JUMPS;) {
        for (u32 b = 0; b < BATCH && k < FOREST_MAX_JUMPS; ++b, ++k)
            FGPU_TRY(launch(forest_jump_kernel, dim3(grid), dim3(256), 0, ctx->stream(), parent, n, flags, k));
        u32 f = 0;
        FGPU_TRY(read_u32(ctx, flags + k - 1, &f));
        if (!f) return FGPU_OK;
    }
    set_error("%s: the parent forest did not flatten in %u pointer-jumping steps", who, FOREST_MAX_JUMPS);
    return FGPU_DEVICE;
}

}  // namespace fgpu
