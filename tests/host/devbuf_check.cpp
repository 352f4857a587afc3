// devbuf_check.cpp — what DevBuf of falkordb_amd/csrc/common.hpp frees, and when, alone and as a member of fgpu_tiles
// (tests/test_ownership_cpu.py builds it with the address and undefined-behaviour sanitizers on the host side and runs it as a
// child process).  fgpu_ctx::dev_alloc / dev_free are defined HERE, as a counting malloc / free: the program makes no HIP
// call, so it runs without a GPU.  Exits 1 with a message on the first rule that breaks; a block freed twice or never is
// the sanitizer's to report.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <set>
#include <utility>

#include "../../falkordb_amd/csrc/common.hpp"

using namespace fgpu;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s failed (line %d)\n", #cond, __LINE__);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

static std::set<void*> g_live;   // blocks handed out and not yet freed
static int g_allocs = 0, g_frees = 0;

fgpu_info fgpu_ctx::dev_alloc(void** p, size_t bytes) {
    CHECK(bytes > 0);
    *p = malloc(bytes);
    CHECK(*p != nullptr && g_live.insert(*p).second);
    ++g_allocs;
    return FGPU_OK;
}
void fgpu_ctx::dev_free(void* p) {
    CHECK(p != nullptr);                 // a holder never frees "nothing"
    CHECK(g_live.erase(p) == 1);         // ... and never the same block twice
    free(p);
    ++g_frees;
}

// a layout with its first `filled` arrays allocated, in declaration order
static std::unique_ptr<fgpu_tiles> tiles(fgpu_ctx* c, int filled) {
    std::unique_ptr<fgpu_tiles> t(new fgpu_tiles());
    DevBuf<uint32_t>* u32s[] = {&t->item_off, &t->item_group, &t->entries, &t->tile_item, &t->bk_seg_off, &t->bk_entries};
    for (int i = 0; i < filled && i < 6; ++i) CHECK(u32s[i]->alloc(c, 8 + i) == FGPU_OK);
    if (filled == 7) CHECK(t->row_has.alloc(c, 4) == FGPU_OK);
    return t;
}

int main() {
    fgpu_ctx ctx;
    // destruction frees once; an empty holder frees nothing
    {
        DevBuf<u32> a, empty;
        CHECK(a.alloc(&ctx, 16) == FGPU_OK);
        CHECK(a.p != nullptr && a.n == 16 && a.ctx == &ctx && empty.p == nullptr);
        CHECK(g_allocs == 1 && g_frees == 0);
    }
    CHECK(g_frees == 1 && g_live.empty());
    // a count of zero still holds a block (a kernel argument is never a null array), freed like any other
    {
        DevBuf<u64> a;
        CHECK(a.alloc(&ctx, 0) == FGPU_OK && a.p != nullptr && a.n == 0);
    }
    CHECK(g_allocs == 2 && g_frees == 2);
    // take() hands the block out and prevents the free
    {
        void* q;
        {
            DevBuf<u32> a;
            CHECK(a.alloc(&ctx, 4) == FGPU_OK);
            q = a.take();
            CHECK(q != nullptr && a.p == nullptr && a.n == 0);
        }
        CHECK(g_frees == 2 && g_live.count(q) == 1);
        ctx.dev_free(q);
    }
    CHECK(g_allocs == 3 && g_frees == 3);
    // a second alloc frees the first block; release() frees at once and may be repeated
    {
        DevBuf<u32> a;
        CHECK(a.alloc(&ctx, 4) == FGPU_OK);
        void* first = a.p;
        CHECK(a.alloc(&ctx, 32) == FGPU_OK);
        CHECK(g_frees == 4 && g_live.count(first) == 0 && g_live.count(a.p) == 1 && a.n == 32);
        a.release();
        CHECK(g_frees == 5 && a.p == nullptr && a.n == 0);
        a.release();
        CHECK(g_frees == 5);
    }
    CHECK(g_allocs == 5 && g_frees == 5);
    // move construction leaves the source empty: one free in all
    {
        DevBuf<u32> a;
        CHECK(a.alloc(&ctx, 4) == FGPU_OK);
        u32* q = a.p;
        DevBuf<u32> b(std::move(a));
        CHECK(a.p == nullptr && a.n == 0 && b.p == q && b.n == 4 && b.ctx == &ctx && g_frees == 5);
    }
    CHECK(g_allocs == 6 && g_frees == 6);
    // move assignment frees the target's old block at once and leaves the source empty; onto itself: nothing happens
    {
        DevBuf<u32> a, b;
        CHECK(a.alloc(&ctx, 4) == FGPU_OK && b.alloc(&ctx, 8) == FGPU_OK);
        u32 *qa = a.p, *qb = b.p;
        b = std::move(a);
        CHECK(g_frees == 7 && g_live.count(qb) == 0 && g_live.count(qa) == 1);
        CHECK(a.p == nullptr && a.n == 0 && b.p == qa && b.n == 4);
        DevBuf<u32>& self = b;
        b = std::move(self);
        CHECK(b.p == qa && b.n == 4 && g_frees == 7);
        // into an empty holder (how a builder attaches an index), and an empty one moved over a full one
        DevBuf<u32> c;
        c = std::move(b);
        CHECK(c.p == qa && b.p == nullptr && g_frees == 7);
        c = DevBuf<u32>();
        CHECK(c.p == nullptr && g_frees == 8);
    }
    CHECK(g_allocs == 8 && g_frees == 8 && g_live.empty());
    // a layout frees exactly the arrays it holds: all seven, or the two a failed build got to
    {
        std::unique_ptr<fgpu_tiles> t = tiles(&ctx, 7);
        CHECK(g_allocs == 15 && g_frees == 8);
    }
    CHECK(g_frees == 15 && g_live.empty());
    {
        std::unique_ptr<fgpu_tiles> t = tiles(&ctx, 2);
        CHECK(g_allocs == 17);
    }
    CHECK(g_frees == 17 && g_live.empty());
    // a rebuild: one layout moved over another frees the old one's blocks once, at the move
    {
        std::unique_ptr<fgpu_tiles> held = tiles(&ctx, 5), fresh = tiles(&ctx, 7);
        const uint32_t* kept = fresh->entries.p;
        CHECK(g_allocs == 29 && g_frees == 17);
        held = std::move(fresh);
        CHECK(g_frees == 22 && fresh == nullptr && held->entries.p == kept && g_live.size() == 7);
    }
    CHECK(g_allocs == 29 && g_frees == 29 && g_live.empty());
    printf("ok\n");
    return 0;
}
