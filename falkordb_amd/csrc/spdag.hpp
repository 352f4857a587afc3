// spdag.hpp — the device code fgpu_shortest_dag (spdag.hip) and fgpu_shortest_dag_batch (spdag_batch.hip) share: the "none"
// level, the depth of a DAG pair, and the one-workgroup sort that orders up to SD_SORT_MAX pairs and writes the result columns.
#pragma once
#include "algo.hpp"

namespace fgpu {

constexpr u32 SD_NONE = 0xFFFFFFFFu;

// the depth of a DAG pair: its from-vertex' forward level where set, else L minus its backward level
struct SdDepth {
    const u32* df;
    const u32* db;
    u32 L;
    __device__ u64 operator()(u32, u32 r, u32) const { return df[r] != SD_NONE ? df[r] : L - db[r]; }
};

constexpr u32 SD_SORT_MAX = 4096;   // pairs the one-workgroup sort takes: 32 KiB of keys in LDS

// k <= SD_SORT_MAX pairs, one workgroup of 256 threads, s_key its SD_SORT_MAX keys of LDS: sorts the keys from << 32 | to
// (bitonic over the next power of two, the padding keys all ones: no vertex id is 0xFFFFFFFF) and writes the three result
// columns in that order
__device__ __forceinline__ void sd_sort_block(u64* s_key, const u32* __restrict__ prow, const u32* __restrict__ pcol, u32 k,
                                              SdDepth depth, u64* __restrict__ ofrom, u64* __restrict__ oto,
                                              u64* __restrict__ odepth) {
    u32 m = 1;
    while (m < k) m <<= 1;
    for (u32 i = threadIdx.x; i < m; i += 256) s_key[i] = i < k ? ((u64)prow[i] << 32) | pcol[i] : ~0ull;
    __syncthreads();
    for (u32 size = 2; size <= m; size <<= 1) {
        for (u32 stride = size >> 1; stride; stride >>= 1) {
            for (u32 t = threadIdx.x; t < (m >> 1); t += 256) {
                const u32 lo = 2 * t - (t & (stride - 1)), hi = lo + stride;   // the t-th index with bit `stride` clear, its partner
                const bool up = (lo & size) == 0;
                const u64 a = s_key[lo], b = s_key[hi];
                if ((a > b) == up) { s_key[lo] = b; s_key[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (u32 i = threadIdx.x; i < k; i += 256) {
        const u64 key = s_key[i];
        const u32 r = (u32)(key >> 32), c = (u32)key;
        ofrom[i] = r;
        oto[i] = c;
        odepth[i] = depth(i, r, c);
    }
}

}  // namespace fgpu
