// matref_check.cpp — what MatRef of falkordb_amd/csrc/common.hpp releases, and when (tests/test_ownership_cpu.py builds it with
// the address and undefined-behaviour sanitizers on the host side and runs it as a child process).  mat_release is defined
// HERE, as a counter: the program makes no HIP call, so it runs without a GPU.  Exits 1 with a message on the first rule that
// breaks.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

#include "../../falkordb_amd/csrc/common.hpp"

using namespace fgpu;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s failed (line %d)\n", #cond, __LINE__);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

static std::map<fgpu_mat*, int> g_released;   // how often each snapshot was released
static int g_total = 0;

namespace fgpu {
void mat_release(fgpu_mat* m) {
    CHECK(m != nullptr);   // the holder never releases "nothing"
    ++g_released[m];
    ++g_total;
}
}  // namespace fgpu

// stand-ins for snapshots: only their addresses are used
static char g_slot[64];
static fgpu_mat* mat(int i) { return reinterpret_cast<fgpu_mat*>(&g_slot[i]); }
static int released(int i) { return g_released[mat(i)]; }

int main() {
    // destruction releases once; an empty holder releases nothing
    {
        MatRef a(mat(0));
        MatRef empty;
        CHECK(a.get() == mat(0) && a.m == mat(0) && empty.get() == nullptr);
        CHECK(g_total == 0);
    }
    CHECK(released(0) == 1 && g_total == 1);
    // a builder fills it through &ref.m
    {
        MatRef a;
        *(&a.m) = mat(1);
        CHECK(a.get() == mat(1));
    }
    CHECK(released(1) == 1 && g_total == 2);
    // release() hands the pointer out and prevents the release
    {
        MatRef a(mat(2));
        fgpu_mat* q = a.release();
        CHECK(q == mat(2) && a.get() == nullptr);
    }
    CHECK(released(2) == 0 && g_total == 2);
    // reset() releases the old pointer at once and holds the new one; reset() of an empty holder releases nothing
    {
        MatRef a(mat(3));
        a.reset(mat(4));
        CHECK(released(3) == 1 && released(4) == 0 && a.get() == mat(4));
        a.reset();
        CHECK(released(4) == 1 && a.get() == nullptr);
        a.reset();
        CHECK(g_total == 4);
    }
    CHECK(g_total == 4);
    // move construction leaves the source empty: one release in all
    {
        MatRef a(mat(5));
        MatRef b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == mat(5) && released(5) == 0);
    }
    CHECK(released(5) == 1 && g_total == 5);
    // move assignment releases the target's old pointer at once and leaves the source empty
    {
        MatRef a(mat(6)), b(mat(7));
        b = std::move(a);
        CHECK(released(7) == 1 && released(6) == 0);
        CHECK(a.get() == nullptr && b.get() == mat(6));
        MatRef& self = b;
        b = std::move(self);   // onto itself: nothing happens
        CHECK(b.get() == mat(6) && released(6) == 0);
    }
    CHECK(released(6) == 1 && released(7) == 1 && g_total == 7);
    // a vector that grows (reallocating on the way) releases each element exactly once, when it goes
    {
        std::vector<MatRef> v;
        for (int i = 8; i < 40; ++i) {
            MatRef e(mat(i));
            v.push_back(std::move(e));
        }
        CHECK(g_total == 7);
        for (int i = 8; i < 40; ++i) CHECK(v[i - 8].get() == mat(i));
    }
    for (int i = 8; i < 40; ++i) CHECK(released(i) == 1);
    CHECK(g_total == 7 + 32);
    printf("ok\n");
    return 0;
}
