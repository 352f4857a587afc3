// sort_plan.hpp — the shape decisions of the stable counting sorts of transpose.hip: the digit split and block geometry of the
// two-level form (ks_*), the digit widths of the LDS-staged form (kp_*) and the sizes its host loop derives from them.  Plain
// C++17: no HIP, nothing of common.hpp, so a host program walks the whole domain (tests/host/sort_plan_check.cpp).  The
// kernels take KsGeom by value and share nothing else with this header.
#pragma once
#include <stdint.h>

#include <stddef.h>

namespace fgpu {

constexpr uint32_t KS_MAX_BUCKETS = 8192;      // pass-1 LDS cursors: 32 KiB
constexpr uint32_t KS_MAX_WB = 13;             // pass-2 LDS counters: 4 quarters x 2^13 x 4 B = 128 KiB
constexpr uint32_t KP_EB = 2048;               // entries per block of the staged form
constexpr uint32_t KP_MAX_D = 512;             // buckets a level of the staged form

struct KsGeom {
    uint32_t wb;     // low-digit bits
    uint32_t B;      // buckets
    uint32_t bbits;  // ballots needed to tell buckets apart
    uint32_t EB;     // entries per pass-1 block
    uint32_t nblk;   // pass-1 blocks
};

// bits of a key space: the smallest kb in 1 .. 32 with 2^kb >= nkeys (32 past that)
inline uint32_t sort_key_bits(uint64_t nkeys) {
    uint32_t kb = 1;
    while (kb < 32 && (1ull << kb) < nkeys) ++kb;
    return kb;
}

// geometry of the two-level form for n pairs over nkeys keys; false = more than KS_MAX_BUCKETS buckets would be needed.
// wb_override: the experiment knob (option "transpose_wb"), low-digit bits, 0 = pick
inline bool ks_geometry(uint64_t n, uint64_t nkeys, int wb_override, KsGeom& g) {
    const uint32_t kb = sort_key_bits(nkeys);
    // split the key bits between the two digits so that neither LDS footprint starves its kernel of wavefronts:
    // pass 1 keeps B x 4 B per single-wavefront workgroup, pass 2 keeps 4 x 2^wb x 4 B per 4-wavefront workgroup
    // Sweep at 2^22 keys (RMAT-22, tools/transpose_wb_sweep.py; count / scatter / bucket ms): wb 10: .29 / 1.38 / .86;
    // 11: .18 / 1.46 / .99; 12: .13 / 1.01 / 1.23; 13: .11 / .66 / 2.26 — fewer pass-1 buckets mean longer runs per
    // bucket (the scattered 8 B pairs combine into lines before they leave L2 / MALL), more pass-2 keys mean LDS
    // counters that leave one workgroup per CU.  Smaller pass-1 blocks (4096, 2048 entries) changed nothing.
    uint32_t wb = kb > 22 ? kb - 12 : (kb > 12 ? 12 : (kb > 11 ? 11 : 8));   // 2^22 keys: 1024 x 4096; 2^24: 4096 x 4096; 2^26: 8192 x 8192
    if (wb < 8) wb = 8;                                // a pass-2 thread owns 2^wb / 256 keys
    if (kb > wb + 13) wb = kb - 13;
    if (wb_override >= 8 && wb_override <= (int)KS_MAX_WB && (uint32_t)wb_override + 13 >= kb) wb = (uint32_t)wb_override;
    if (wb > KS_MAX_WB) wb = KS_MAX_WB;
    const uint64_t B = (nkeys + (1ull << wb) - 1) >> wb;
    if (B > KS_MAX_BUCKETS) return false;      // > 2^26 keys: three digits would be needed
    g.wb = wb;
    g.B = (uint32_t)(B ? B : 1);
    g.bbits = 0;
    while ((1u << g.bbits) < g.B) ++g.bbits;
    uint64_t eb = 16384;
    while ((n + eb - 1) / eb > 4096) eb <<= 1;  // the count matrix stays <= B x 4096

    g.EB = (uint32_t)eb;
    g.nblk = (uint32_t)((n + eb - 1) / eb);
    if (g.nblk == 0) g.nblk = 1;
    return true;
}

// digit widths of the staged form, most significant first: as few levels as 9 bits a level allow, at least ... balanced
// (w holds 8 entries)
inline int kp_widths(uint64_t nkeys, uint32_t* w) {
    const uint32_t kb = sort_key_bits(nkeys);
    int L = (int)((kb + 8) / 9);
    if (L < 1) L = 1;
    if (kb >= 17 && L < 3) L = 3;                 // (runs of whole lines need <= 512 buckets a level; 3 levels from 2^17 keys)
    if ((uint32_t)L > kb) L = (int)kb;
    // the wider digits last: a level's runs are KP_EB / D entries long, and the last level moves 4-byte values in segments
    // that mostly fit one block (written as one contiguous piece whatever D is)
    for (int l = 0; l < L; ++l) w[l] = kb / L + ((uint32_t)(L - 1 - l) < kb % L ? 1u : 0u);
    return L;
}

// what the staged form accepts: the block tables index n + KP_EB entries and nkeys + 1 key pointers with 32 bits
inline bool kp_accepts(uint64_t n, uint64_t nkeys) {
    return n != 0 && n < 0xFFFFFFFFull - KP_EB && nkeys != 0 && nkeys <= (1ull << 31);
}

// ---- sizes the staged form's host loop derives from the widths; a level with S segments has at most n / KP_EB + S blocks
// the most segments any level starts from: 2^(bits of all levels but the last)
inline uint64_t kp_s_max(const uint32_t* w, int L) {
    uint64_t S_max = 1;
    uint32_t done = 0;
    for (int l = 0; l + 1 < L; ++l) { done += w[l]; S_max = 1ull << done; }
    return S_max;
}
// block descriptors allocated once for all levels
inline uint64_t kp_nb_top(uint64_t n, uint64_t S_max) { return n / KP_EB + 9 + S_max; }
// blocks (= workgroups) of a level with S segments, a multiple of 8
inline uint64_t kp_nb_max(uint64_t n, uint32_t S) { return (n / KP_EB + 1 + S + 7) & ~7ull; }
// counters of a level: D per block and the total
inline size_t kp_ncnt(uint32_t D, uint64_t nb_max) { return (size_t)D * nb_max + 1; }
// dynamic LDS of the scatter kernel: KP_EB staged pairs, then per-wavefront counters / cursors and the bucket bases
inline size_t kp_scatter_lds_bytes(uint32_t D) { return ((size_t)2 * KP_EB + (size_t)6 * D) * sizeof(uint32_t); }

}  // namespace fgpu
