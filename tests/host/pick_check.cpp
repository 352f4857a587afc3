// pick_check.cpp — what pick<...>() and pick(bool) of falkordb_amd/csrc/common.hpp hand their callable, on the host
// (tests/test_launch_cpu.py builds it with the address and undefined-behaviour sanitizers on the host side and runs it as a
// child process).  It makes no HIP call, so it runs without a GPU.  Exits 1 with a message on the first rule that breaks.
#include <stdio.h>
#include <stdlib.h>

#include "../../falkordb_amd/csrc/common.hpp"

using namespace fgpu;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s failed (line %d)\n", #cond, __LINE__);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// the constant pick<1, 2, 4, 8> hands over for `v`, and how often it called
static int picked(int v, int* calls) {
    int got = -1000;
    const fgpu_info i = pick<1, 2, 4, 8>(v, [&](auto c) {
        static_assert(std::is_same<decltype(c), std::integral_constant<int, decltype(c)::value>>::value, "an integral_constant<int, V>");
        got = decltype(c)::value;
        ++*calls;
        return FGPU_OK;
    });
    CHECK(i == FGPU_OK);
    return got;
}

int main() {
    // each listed value reaches its own constant, an unlisted one the last; the callable runs exactly once
    for (int v : {1, 2, 4, 8}) {
        int calls = 0;
        CHECK(picked(v, &calls) == v);
        CHECK(calls == 1);
    }
    for (int v : {3, 0, -1}) {
        int calls = 0;
        CHECK(picked(v, &calls) == 8);
        CHECK(calls == 1);
    }
    // a bool reaches true_type / false_type
    for (bool b : {true, false}) {
        int calls = 0;
        bool got = !b;
        CHECK(pick(b, [&](auto c) {
            static_assert(std::is_same<decltype(c), std::true_type>::value || std::is_same<decltype(c), std::false_type>::value, "a bool constant");
            got = decltype(c)::value;
            ++calls;
            return FGPU_OK;
        }) == FGPU_OK);
        CHECK(got == b && calls == 1);
    }
    // nested picks compose: every pair of run-time values names its own pair of constants, once
    for (bool b : {true, false})
        for (int v : {1, 2, 0, 7}) {
            int calls = 0, gv = -1000;
            bool gb = !b;
            CHECK(pick(b, [&](auto cb) {
                return pick<1, 2, 0>(v, [&](auto cv) {
                    gb = decltype(cb)::value;
                    gv = decltype(cv)::value;
                    ++calls;
                    return FGPU_OK;
                });
            }) == FGPU_OK);
            CHECK(gb == b && gv == (v == 7 ? 0 : v) && calls == 1);
        }
    // what the callable returns is what pick returns, through every level
    for (fgpu_info want : {FGPU_OK, FGPU_DEVICE, FGPU_OOM}) {
        CHECK((pick<1, 2>(2, [&](auto) { return want; })) == want);
        CHECK((pick<1, 2>(5, [&](auto) { return want; })) == want);
        CHECK(pick(true, [&](auto) { return want; }) == want);
        CHECK(pick(false, [&](auto) { return pick<4, 8>(4, [&](auto) { return want; }); }) == want);
    }
    printf("ok\n");
    return 0;
}
