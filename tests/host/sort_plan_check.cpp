// sort_plan_check.cpp — walks the shape decisions of the stable counting sorts (falkordb_amd/csrc/sort_plan.hpp) over their whole
// domain on the host: key spaces 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 32 and 2^32 - 2, entry counts 1, 4095, 4096, 4097, 2^24, 2^31,
// the largest the staged form accepts (2^32 - 2 - KP_EB) and the first it refuses, every "transpose_wb" override from -1 to 32.
// Checked:
//   kp_widths     1 <= L <= 8 (the caller's array); the widths sum to the key bits; 1 <= w, 2^w <= KP_MAX_D; L >= 3 from 17 bits;
//                 L == 4 exactly for 28 .. 32 bits; the widths never decrease; the splits DESIGN.md names
//   staged domain (kp_accepts, nkeys >= 2) every quantity a kernel or dim3 takes as 32 bits stays below 2^32 — nb_max, ncnt, S x D,
//                 nkeys + 1 —, the tables allocated once (nb_top descriptors, dmax x nb_top counters) hold every level's, a level's
//                 block bound covers n / KP_EB + S, and the scatter kernel's LDS stays below 64 KiB
//   ks_geometry   accepts exactly nkeys <= 2^26; there 8 <= wb <= 13, B = ceil(nkeys / 2^wb) <= 8192, 2^(bbits - 1) < B <= 2^bbits,
//                 EB a power of two >= 16384, nblk <= 4096, EB x nblk >= n; the override is honoured only for 8 <= o <= 13 with
//                 o + 13 >= key bits; the (wb, buckets) pairs of 22 .. 26 bits
// Prints "ok <combinations checked>" and exits 0, or says what failed and exits 1.  Built with -fsanitize=address,undefined by
// tests/test_sort_plan_cpu.py and run as a child process.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../falkordb_amd/csrc/sort_plan.hpp"

using namespace fgpu;
typedef uint32_t u32;
typedef uint64_t u64;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            exit(1);                                      \
        }                                                 \
    } while (0)

static const u64 TWO32 = 1ull << 32;
static u64 checked = 0;

static u32 bits_of(u64 nkeys) {   // the smallest kb <= 32 with 2^kb >= nkeys, at least 1
    for (u32 kb = 1; kb < 32; ++kb)
        if ((1ull << kb) >= nkeys) return kb;
    return 32;
}

static void check_widths(u64 nkeys) {
    u32 w[10];
    for (u32& x : w) x = 0xDEADu;
    const int L = kp_widths(nkeys, w);
    const u32 kb = bits_of(nkeys);
    CHECK(L >= 1 && L <= 8, "nkeys %llu: L = %d", (unsigned long long)nkeys, L);
    CHECK(w[8] == 0xDEADu && w[9] == 0xDEADu, "nkeys %llu: wrote past 8 widths", (unsigned long long)nkeys);
    u32 sum = 0;
    for (int l = 0; l < L; ++l) {
        CHECK(w[l] >= 1 && (1u << w[l]) <= KP_MAX_D, "nkeys %llu: w[%d] = %u", (unsigned long long)nkeys, l, w[l]);
        if (l) CHECK(w[l] >= w[l - 1], "nkeys %llu: w[%d] = %u after %u", (unsigned long long)nkeys, l, w[l], w[l - 1]);
        sum += w[l];
    }
    CHECK(sum == kb, "nkeys %llu: widths sum to %u, key bits %u", (unsigned long long)nkeys, sum, kb);
    if (kb >= 17) CHECK(L >= 3, "nkeys %llu: %d levels at %u bits", (unsigned long long)nkeys, L, kb);
    CHECK((L == 4) == (kb >= 28), "nkeys %llu: %d levels at %u bits", (unsigned long long)nkeys, L, kb);
    ++checked;
}

static void check_split(u64 nkeys, std::vector<u32> want) {
    u32 w[8];
    const int L = kp_widths(nkeys, w);
    CHECK((size_t)L == want.size(), "nkeys %llu: %d levels", (unsigned long long)nkeys, L);
    for (int l = 0; l < L; ++l) CHECK(w[l] == want[l], "nkeys %llu: w[%d] = %u", (unsigned long long)nkeys, l, w[l]);
    ++checked;
}

static void check_staged(u64 n, u64 nkeys) {
    const bool want = n >= 1 && n < TWO32 - 1 - KP_EB && nkeys >= 1 && nkeys <= (1ull << 31);
    CHECK(kp_accepts(n, nkeys) == want, "n %llu nkeys %llu: accepted %d", (unsigned long long)n, (unsigned long long)nkeys,
          (int)kp_accepts(n, nkeys));
    ++checked;
    if (!want || nkeys < 2) return;
    u32 w[8];
    const int L = kp_widths(nkeys, w);
    const u64 S_max = kp_s_max(w, L), nb_top = kp_nb_top(n, S_max);
    u32 dmax = 0, done = 0;
    for (int l = 0; l < L; ++l) dmax = dmax > (1u << w[l]) ? dmax : (1u << w[l]);
    CHECK(nkeys + 1 < TWO32, "nkeys + 1");
    CHECK(kp_scatter_lds_bytes(dmax) < 65536 && kp_scatter_lds_bytes(dmax) >= (2 * KP_EB + 6 * dmax) * 4u, "LDS of D = %u", dmax);
    for (int l = 0; l < L; ++l) {
        const u64 S = 1ull << done, D = 1ull << w[l];
        CHECK(S <= S_max && S < TWO32, "n %llu nkeys %llu level %d: S %llu, S_max %llu", (unsigned long long)n,
              (unsigned long long)nkeys, l, (unsigned long long)S, (unsigned long long)S_max);
        const u64 nb_max = kp_nb_max(n, (u32)S);
        const u64 ncnt = kp_ncnt((u32)D, nb_max);
        CHECK(nb_max >= n / KP_EB + 1 + S && nb_max % 8 == 0, "level %d: nb_max %llu", l, (unsigned long long)nb_max);
        CHECK(nb_max < TWO32 && nb_max <= nb_top, "n %llu nkeys %llu level %d: nb_max %llu, nb_top %llu", (unsigned long long)n,
              (unsigned long long)nkeys, l, (unsigned long long)nb_max, (unsigned long long)nb_top);
        CHECK(ncnt == D * nb_max + 1 && ncnt < TWO32 && ncnt <= (u64)dmax * nb_top + 2, "n %llu nkeys %llu level %d: ncnt %llu",
              (unsigned long long)n, (unsigned long long)nkeys, l, (unsigned long long)ncnt);
        CHECK(S * D < TWO32 && (l + 1 < L ? S * D <= S_max : S * D >= nkeys), "n %llu nkeys %llu level %d: S x D = %llu",
              (unsigned long long)n, (unsigned long long)nkeys, l, (unsigned long long)(S * D));
        done += w[l];
        ++checked;
    }
}

static void check_geometry(u64 n, u64 nkeys) {
    const u32 kb = bits_of(nkeys);
    KsGeom base = {77, 77, 77, 77, 77};
    const bool ok0 = ks_geometry(n, nkeys, 0, base);
    CHECK(ok0 == (nkeys <= (1ull << 26)), "n %llu nkeys %llu: accepted %d", (unsigned long long)n, (unsigned long long)nkeys, (int)ok0);
    for (int o = -1; o <= 32; ++o) {
        KsGeom g = {77, 77, 77, 77, 77};
        const bool ok = ks_geometry(n, nkeys, o, g);
        CHECK(ok == ok0, "n %llu nkeys %llu override %d: accepted %d", (unsigned long long)n, (unsigned long long)nkeys, o, (int)ok);
        ++checked;
        if (!ok) continue;
        const bool honoured = o >= 8 && o <= 13 && (u32)o + 13 >= kb;
        if (honoured) CHECK(g.wb == (u32)o, "nkeys %llu override %d: wb %u", (unsigned long long)nkeys, o, g.wb);
        else CHECK(g.wb == base.wb, "nkeys %llu override %d not to be honoured: wb %u, picked %u", (unsigned long long)nkeys, o, g.wb, base.wb);
        CHECK(g.wb >= 8 && g.wb <= KS_MAX_WB && KS_MAX_WB == 13, "nkeys %llu override %d: wb %u", (unsigned long long)nkeys, o, g.wb);
        const u64 B = (nkeys + (1ull << g.wb) - 1) >> g.wb;
        CHECK(g.B == B && B >= 1 && B <= KS_MAX_BUCKETS && KS_MAX_BUCKETS == 8192, "nkeys %llu override %d: B %u", (unsigned long long)nkeys, o, g.B);
        CHECK(g.bbits <= 13 && g.B <= (1u << g.bbits) && (g.bbits == 0 ? g.B == 1 : g.B > (1u << (g.bbits - 1))),
              "nkeys %llu override %d: B %u bbits %u", (unsigned long long)nkeys, o, g.B, g.bbits);
        CHECK(g.EB >= 16384 && (g.EB & (g.EB - 1)) == 0, "n %llu: EB %u", (unsigned long long)n, g.EB);
        CHECK(g.nblk >= 1 && g.nblk <= 4096 && (u64)g.EB * g.nblk >= n, "n %llu: EB %u nblk %u", (unsigned long long)n, g.EB, g.nblk);
        CHECK(g.EB == 16384 || (u64)(g.EB / 2) * 4096 < n, "n %llu: EB %u is not the smallest", (unsigned long long)n, g.EB);
    }
}

static void check_pair(u64 nkeys, u32 wb, u32 B) {
    KsGeom g;
    CHECK(ks_geometry(5000, nkeys, 0, g) && g.wb == wb && g.B == B, "nkeys %llu: wb %u, B %u", (unsigned long long)nkeys, g.wb, g.B);
    ++checked;
}

int main() {
    std::vector<u64> keys, ns = {1, 4095, 4096, 4097, 1ull << 24, 1ull << 31, TWO32 - 2 - KP_EB, TWO32 - 1 - KP_EB, TWO32 - 2};
    for (u32 k = 1; k <= 32; ++k)
        for (int d = -1; d <= 1; ++d) keys.push_back((1ull << k) + (u64)(int64_t)d);
    keys.push_back(TWO32 - 2);
    CHECK(KP_EB == 2048 && KP_MAX_D == 512, "constants");
    for (u64 nkeys : keys) {
        check_widths(nkeys);
        for (u64 n : ns) {
            check_staged(n, nkeys);
            check_geometry(n, nkeys);
        }
    }
    check_staged(0, 1000);
    check_staged(5000, 0);
    // the splits and geometries the design notes name
    check_split(1ull << 16, {8, 8});
    check_split((1ull << 16) + 1, {5, 6, 6});
    check_split(1ull << 22, {7, 7, 8});
    check_split((1ull << 24) + 1, {8, 8, 9});
    check_split(1ull << 26, {8, 9, 9});
    check_split((1ull << 26) + 1, {9, 9, 9});
    check_split(1ull << 27, {9, 9, 9});
    check_split((1ull << 27) + 1, {7, 7, 7, 7});
    check_split(1ull << 31, {7, 8, 8, 8});
    check_split(TWO32 - 2, {8, 8, 8, 8});
    check_pair(1ull << 22, 12, 1u << 10);
    check_pair(1ull << 23, 11, 1u << 12);
    check_pair(1ull << 24, 12, 1u << 12);
    check_pair((1ull << 24) + 1, 13, 2049);
    check_pair(1ull << 25, 13, 1u << 12);
    check_pair(1ull << 26, 13, 1u << 13);
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
