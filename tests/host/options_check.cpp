// options_check.cpp — walks the option table of falkordb_amd/csrc/options.hpp on the host (tests/test_options_cpu.py builds it
// with the address and undefined-behaviour sanitizers and runs it as a child process).  Prints "name kind lo hi default" per
// row; exits 1 with a message on the first rule a row breaks.
#include <stdio.h>
#include <stdlib.h>

#include "../../falkordb_amd/csrc/options.hpp"

using namespace fgpu;

static const char* g_row = "";
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s: %s failed (line %d)\n", g_row, #cond, __LINE__); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

// `v` is stored and read back as `want`
static void accepted(const OptRow& r, int64_t v, int64_t want) {
    fgpu_options o;
    CHECK(opt_accepts(r, v));
    opt_store(o, r, v);
    CHECK(opt_load(o, r) == want);
}

// what fgpu_set_option does with a value the row refuses: nothing is stored
static void rejected(const OptRow& r, int64_t v) {
    fgpu_options o;
    const int64_t before = opt_load(o, r);
    CHECK(!opt_accepts(r, v));
    CHECK(opt_load(o, r) == before);
}

int main() {
    static const char* const kinds[] = {"bool", "range", "pow2"};
    const fgpu_options defaults;
    for (const OptRow& r : OPTIONS) {
        g_row = r.name;
        CHECK((r.i32 != nullptr) != (r.i64 != nullptr));
        CHECK(opt_find(r.name) == &r);   // names are unique: the search finds this row, not an earlier one
        const int64_t def = opt_load(defaults, r);
        printf("%s %s %lld %lld %lld\n", r.name, kinds[r.kind], (long long)r.lo, (long long)r.hi, (long long)def);
        accepted(r, def, def);
        if (r.kind == OPT_BOOL) {
            CHECK(r.lo == 0 && r.hi == 1);
            accepted(r, 7, 1);
            accepted(r, -1, 1);
            accepted(r, 0, 0);
            continue;
        }
        accepted(r, r.lo, r.lo);
        accepted(r, r.hi, r.hi);
        if (r.lo > INT64_MIN) rejected(r, r.lo - 1);
        if (r.hi < INT64_MAX) rejected(r, r.hi + 1);
        if (r.i32) {   // an int field: nothing past its range may be accepted
            CHECK(r.lo >= INT32_MIN && r.hi <= INT32_MAX);
            rejected(r, (int64_t)INT32_MAX + 1);
            rejected(r, 1ll << 32);
        }
        if (r.kind == OPT_POW2) {
            CHECK(r.lo >= 1);
            CHECK((r.lo & (r.lo - 1)) == 0 && (r.hi & (r.hi - 1)) == 0);
            if (2 * r.lo < r.hi) accepted(r, 2 * r.lo, 2 * r.lo);
            for (int64_t v = r.lo + 1; v < r.hi; ++v)
                if (v & (v - 1)) rejected(r, v);
        }
    }
    g_row = "tiled_u";
    rejected(*opt_find("tiled_u"), 3);
    g_row = "expand_scan_rows";
    rejected(*opt_find("expand_scan_rows"), 96);
    g_row = "expand_scan_min";
    rejected(*opt_find("expand_scan_min"), 1ll << 31);   // the field is an int
    g_row = "bfs_pb_min_edges";
    accepted(*opt_find("bfs_pb_min_edges"), 1ll << 40, 1ll << 40);
    g_row = "unknown names";
    CHECK(opt_find("no_such_option") == nullptr);
    CHECK(opt_find("") == nullptr);
    CHECK(opt_find("lds_limit") == nullptr);      // filled by fgpu_init, not settable
    CHECK(opt_find("transpose_wb") == nullptr);   // a special case of fgpu_set_option, not a row
    CHECK(opt_find("sssp_delta_log2") == nullptr);   // likewise: an exponent or auto: no row kind fits
    CHECK(opt_find("tiled_u ") == nullptr);
    return 0;
}
