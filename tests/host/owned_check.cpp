// owned_check.cpp — what SnapshotRef, PlanRef and EngineBuf<T> of falkordb_amd/host/owned.hpp give back, and when
// (tests/test_ownership_cpu.py builds it with the address and undefined-behaviour sanitizers on the host side and runs it as a
// child process).  The four engine functions the owners call are defined HERE: the two handle frees as counters over plain
// addresses, fgpu_host_alloc over malloc (failing on demand) and fgpu_free over free, so a block freed twice or never is the
// sanitizer's to report.  The program makes no HIP call, so it runs without a GPU.  Exits 1 with a message on the first rule
// that breaks.
#include <stdio.h>
#include <stdlib.h>

#include <map>
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

static std::map<void*, int> g_freed;   // how often each handle was freed
static int g_handle_frees = 0;         // fgpu_mat_free + fgpu_bfs_plan_free calls
static int g_blocks_live = 0;          // blocks of fgpu_host_alloc / malloc not yet given to fgpu_free
static int g_block_frees = 0;
static fgpu_ctx* g_last_ctx = nullptr; // the context of the last fgpu_free
static bool g_alloc_fails = false;

fgpu_info fgpu_mat_free(fgpu_mat* m) {
    CHECK(m != nullptr);   // an owner never frees "nothing"
    ++g_freed[m];
    ++g_handle_frees;
    return FGPU_OK;
}
fgpu_info fgpu_bfs_plan_free(fgpu_bfs_plan* p) {
    CHECK(p != nullptr);
    ++g_freed[p];
    ++g_handle_frees;
    return FGPU_OK;
}
fgpu_info fgpu_host_alloc(fgpu_ctx* ctx, uint64_t bytes, void** out) {
    CHECK(ctx && out && bytes);
    if (g_alloc_fails) return FGPU_OOM;
    *out = malloc(bytes);
    ++g_blocks_live;
    return FGPU_OK;
}
void fgpu_free(fgpu_ctx* ctx, void* p) {
    CHECK(p != nullptr);
    g_last_ctx = ctx;
    --g_blocks_live;
    ++g_block_frees;
    free(p);
}
namespace falkor {
void check(fgpu_info i, const char* where) {
    if (i != FGPU_OK) throw std::runtime_error(where);
}
}  // namespace falkor

// stand-ins for handles and contexts: only their addresses are used
static char g_slot[64];
template <typename H>
static H* handle(int i) { return reinterpret_cast<H*>(&g_slot[i]); }
static fgpu_ctx* ctx(int i) { return reinterpret_cast<fgpu_ctx*>(&g_slot[i]); }
static int freed(int i) { return g_freed[&g_slot[i]]; }

template <typename R, typename H>
static void check_handle_owner() {
    g_freed.clear();
    g_handle_frees = 0;
    // destruction frees once; an empty owner frees nothing
    {
        R a(handle<H>(0));
        R empty;
        CHECK(a.get() == handle<H>(0) && empty.get() == nullptr);
        CHECK(g_handle_frees == 0);
    }
    CHECK(freed(0) == 1 && g_handle_frees == 1);
    // the engine fills it through out(); destruction then frees once
    {
        R a;
        *a.out() = handle<H>(1);
        CHECK(a.get() == handle<H>(1));
    }
    CHECK(freed(1) == 1 && g_handle_frees == 2);
    // release() hands the handle out and prevents the free
    {
        R a(handle<H>(2));
        CHECK(a.release() == handle<H>(2) && a.get() == nullptr);
    }
    CHECK(freed(2) == 0 && g_handle_frees == 2);
    // reset() frees the old handle at once and holds the new one; reset() of an empty owner frees nothing
    {
        R a(handle<H>(3));
        a.reset(handle<H>(4));
        CHECK(freed(3) == 1 && freed(4) == 0 && a.get() == handle<H>(4));
        a.reset();
        CHECK(freed(4) == 1 && a.get() == nullptr);
        a.reset();
        CHECK(g_handle_frees == 4);
    }
    CHECK(g_handle_frees == 4);
    // move construction leaves the source empty: one free in all
    {
        R a(handle<H>(5));
        R b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == handle<H>(5) && freed(5) == 0);
    }
    CHECK(freed(5) == 1 && g_handle_frees == 5);
    // move assignment frees the target's old handle at once and leaves the source empty; onto itself nothing happens
    {
        R a(handle<H>(6)), b(handle<H>(7));
        b = std::move(a);
        CHECK(freed(7) == 1 && freed(6) == 0 && a.get() == nullptr && b.get() == handle<H>(6));
        R& self = b;
        b = std::move(self);
        CHECK(b.get() == handle<H>(6) && freed(6) == 0);
    }
    CHECK(freed(6) == 1 && freed(7) == 1 && g_handle_frees == 7);
    // a vector that grows (reallocating on the way) frees each element exactly once, when it goes
    {
        std::vector<R> v;
        for (int i = 8; i < 40; ++i) {
            R e(handle<H>(i));
            v.push_back(std::move(e));
        }
        CHECK(g_handle_frees == 7);
        for (int i = 8; i < 40; ++i) CHECK(v[i - 8].get() == handle<H>(i));
    }
    for (int i = 8; i < 40; ++i) CHECK(freed(i) == 1);
    CHECK(g_handle_frees == 7 + 32);
    // an exception between out() and the end of the scope still frees
    try {
        R a;
        *a.out() = handle<H>(40);
        check(FGPU_INVALID, "thrown on purpose");
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(freed(40) == 1 && g_handle_frees == 7 + 32 + 1);
}

template <typename T>
static T* block() {   // what the engine hands out through an out-parameter
    ++g_blocks_live;
    return (T*)malloc(4 * sizeof(T));
}

template <typename T>
static void check_engine_buf() {
    CHECK(g_blocks_live == 0);
    g_block_frees = 0;
    // destruction frees once, with the context of construction; an empty owner frees nothing
    {
        EngineBuf<T> a(ctx(1)), empty(ctx(2));
        *a.out() = block<T>();
        a[3] = T(7);
        CHECK(a.p[3] == T(7) && empty.p == nullptr && g_block_frees == 0);
    }
    CHECK(g_block_frees == 1 && g_blocks_live == 0 && g_last_ctx == ctx(1));
    // alloc() takes a pinned block of `count` entries (of one when count is 0) and frees the one held before
    {
        EngineBuf<T> a(ctx(3));
        a.alloc(5, "alloc");
        a[4] = T(1);
        a.alloc(0, "alloc");
        CHECK(g_block_frees == 2 && g_blocks_live == 1 && g_last_ctx == ctx(3));
        a[0] = T(2);
    }
    CHECK(g_block_frees == 3 && g_blocks_live == 0);
    // an alloc() that fails throws and leaves the owner empty, the block held before gone
    {
        EngineBuf<T> a(ctx(4));
        a.alloc(2, "alloc");
        g_alloc_fails = true;
        bool thrown = false;
        try {
            a.alloc(2, "alloc");
        } catch (const std::runtime_error&) {
            thrown = true;
        }
        g_alloc_fails = false;
        CHECK(thrown && a.p == nullptr && g_block_frees == 4);
    }
    CHECK(g_block_frees == 4 && g_blocks_live == 0);
    // release() hands the block out and prevents the free; reset() frees at once, and nothing on an empty owner
    {
        EngineBuf<T> a(ctx(5));
        a.alloc(1, "alloc");
        T* q = a.release();
        CHECK(q && a.p == nullptr);
        a.reset();
        CHECK(g_block_frees == 4);
        *a.out() = q;
        a.reset();
        CHECK(g_block_frees == 5 && a.p == nullptr && g_last_ctx == ctx(5));
    }
    CHECK(g_block_frees == 5 && g_blocks_live == 0);
    // both moves carry the context along and leave the source empty; a self-move does nothing
    {
        EngineBuf<T> a(ctx(6));
        a.alloc(1, "alloc");
        T* qa = a.p;
        EngineBuf<T> b(std::move(a));
        CHECK(a.p == nullptr && b.p == qa && b.ctx == ctx(6));
        EngineBuf<T> c(ctx(7));
        c.alloc(1, "alloc");
        c = std::move(b);
        CHECK(g_block_frees == 6 && g_last_ctx == ctx(7));   // c's old block, to c's old context
        CHECK(b.p == nullptr && c.p == qa && c.ctx == ctx(6));
        EngineBuf<T>& self = c;
        c = std::move(self);
        CHECK(c.p == qa && g_block_frees == 6);
    }
    CHECK(g_block_frees == 7 && g_blocks_live == 0 && g_last_ctx == ctx(6));
    // a vector that grows frees each element exactly once
    {
        std::vector<EngineBuf<T>> v;
        for (int i = 0; i < 32; ++i) {
            EngineBuf<T> e(ctx(8));
            e.alloc(1, "alloc");
            v.push_back(std::move(e));
        }
        CHECK(g_block_frees == 7 && g_blocks_live == 32);
    }
    CHECK(g_block_frees == 7 + 32 && g_blocks_live == 0);
    // an exception between out() and the end of the scope still frees
    try {
        EngineBuf<T> a(ctx(9));
        *a.out() = block<T>();
        check(FGPU_INVALID, "thrown on purpose");
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(g_block_frees == 7 + 32 + 1 && g_blocks_live == 0 && g_last_ctx == ctx(9));
}

int main() {
    check_handle_owner<SnapshotRef, fgpu_mat>();
    check_handle_owner<PlanRef, fgpu_bfs_plan>();
    check_engine_buf<uint64_t>();
    check_engine_buf<double>();
    check_engine_buf<int32_t>();
    check_engine_buf<int64_t>();
    check_engine_buf<float>();
    check_engine_buf<uint16_t>();
    check_engine_buf<uint32_t>();
    printf("ok\n");
    return 0;
}
