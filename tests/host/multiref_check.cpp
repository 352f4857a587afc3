// multiref_check.cpp — what MultiRef of falkordb_amd/host/owned.hpp gives back, and when, in the two shapes the host layer holds
// it: alone, and behind the std::shared_ptr a Tensor and its dup()ed copies share (Tensor::multi_table: a copy that writes drops
// its own reference, the table goes with the last one).  tests/test_expand_edges_cpu.py builds it with the address and
// undefined-behaviour sanitizers on the host side and runs it as a child process.  fgpu_multi_free is defined HERE as a counter
// over plain addresses; the program makes no HIP call, so it runs without a GPU.  Exits 1 with a message on the first rule that
// breaks.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../falkordb_amd/host/owned.hpp"

using namespace falkor;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s failed (line %d)\n", #cond, __LINE__);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

static std::map<void*, int> g_freed;   // how often each table was freed
static int g_frees = 0;

fgpu_info fgpu_multi_free(fgpu_multi* t) {
    CHECK(t != nullptr);   // an owner never frees "nothing"
    ++g_freed[t];
    ++g_frees;
    return FGPU_OK;
}
namespace falkor {
void check(fgpu_info i, const char* where) {
    if (i != FGPU_OK) throw std::runtime_error(where);
}
}  // namespace falkor

static char g_slot[16];
static fgpu_multi* table(int i) { return reinterpret_cast<fgpu_multi*>(&g_slot[i]); }
static int freed(int i) { auto it = g_freed.find(&g_slot[i]); return it == g_freed.end() ? 0 : it->second; }

// the holder of Tensor: copies share, a writer drops its own
struct Holder {
    std::shared_ptr<MultiRef> multi;
};

int main() {
    // alone: destruction frees once, an empty owner and a released one free nothing, a move carries the table over
    {
        MultiRef a(table(0)), empty;
        MultiRef b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == table(0) && g_frees == 0);
        MultiRef c;
        *c.out() = table(1);
        CHECK(c.release() == table(1));
        c = std::move(b);
        CHECK(c.get() == table(0) && g_frees == 0);
        c.reset(table(2));
        CHECK(freed(0) == 1 && g_frees == 1);
    }
    CHECK(freed(2) == 1 && freed(1) == 0 && g_frees == 2);
    // an exception between out() and the end of the scope still frees
    try {
        MultiRef a;
        *a.out() = table(3);
        check(FGPU_INVALID, "after the table was made");
    } catch (const std::runtime_error&) {
    }
    CHECK(freed(3) == 1 && g_frees == 3);
    // shared by copies: the table lives until the last holder drops it, and is freed once
    {
        Holder t;
        t.multi = std::make_shared<MultiRef>();
        *t.multi->out() = table(4);
        Holder dup = t;                        // Tensor::dup copies the holder
        std::vector<Holder> versions(3, t);    // ... and so does a vector of tensors that grows
        t.multi.reset();                       // the writer drops its own reference
        CHECK(g_frees == 3 && dup.multi->get() == table(4));
        t.multi = std::make_shared<MultiRef>();
        *t.multi->out() = table(5);            // ... and builds a table of its own state
        versions.clear();
        CHECK(g_frees == 3);
        dup.multi.reset();
        CHECK(freed(4) == 1 && g_frees == 4);
    }
    CHECK(freed(5) == 1 && g_frees == 5);
    for (auto& kv : g_freed) CHECK(kv.second == 1);
    printf("ok\n");
    return 0;
}
