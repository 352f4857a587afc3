// owned.hpp — the host layer's owners of engine handles.  Every engine call above the C ABI goes through check(), which throws:
// whatever the engine hands out is put into one of these by the call that makes it (through out()), so it goes back on every
// way out.  Move-only, in the shape of the engine's own MatRef / DevBuf.  Includes only fgpu.h and the standard library
// (tests/host/owned_check.cpp builds it over counting stand-ins for the engine's functions).
#pragma once
#include <assert.h>
#include <stddef.h>

#include "../../include/fgpu.h"

namespace falkor {

void check(fgpu_info i, const char* where);   // throws GrbError unless FGPU_OK (matrix.cpp)

// One engine object, given back with Free unless release() handed it on.
template <typename H, fgpu_info (*Free)(H*)>
struct HandleRef {
    H* h = nullptr;
    HandleRef() {}
    explicit HandleRef(H* take) : h(take) {}
    HandleRef(const HandleRef&) = delete;
    HandleRef& operator=(const HandleRef&) = delete;
    HandleRef(HandleRef&& o) noexcept : h(o.release()) {}
    HandleRef& operator=(HandleRef&& o) noexcept { if (this != &o) reset(o.release()); return *this; }
    ~HandleRef() { reset(); }
    void reset(H* take = nullptr) { if (h) (void)Free(h); h = take; }   // the held object is freed NOW
    H* release() { H* q = h; h = nullptr; return q; }
    H* get() const { return h; }
    H** out() { assert(!h); return &h; }   // for the engine's out-parameters: only an empty holder may be filled
};
using SnapshotRef = HandleRef<fgpu_mat, fgpu_mat_free>;        // a snapshot the engine made, until a Matrix shares it
using PlanRef = HandleRef<fgpu_bfs_plan, fgpu_bfs_plan_free>;  // a BFS plan
using MultiRef = HandleRef<fgpu_multi, fgpu_multi_free>;       // a tensor's multi-edge rows resident on the device

// One block that goes back with fgpu_free(ctx, p): a result array of the engine, or a pinned block of fgpu_host_alloc.
template <typename T>
struct EngineBuf {
    fgpu_ctx* ctx;
    T* p = nullptr;
    explicit EngineBuf(fgpu_ctx* c = nullptr) : ctx(c) {}
    EngineBuf(const EngineBuf&) = delete;
    EngineBuf& operator=(const EngineBuf&) = delete;
    EngineBuf(EngineBuf&& o) noexcept : ctx(o.ctx), p(o.release()) {}
    EngineBuf& operator=(EngineBuf&& o) noexcept { if (this != &o) { reset(); ctx = o.ctx; p = o.release(); } return *this; }
    ~EngineBuf() { reset(); }
    void reset() { if (p) fgpu_free(ctx, p); p = nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }
    T** out() { assert(!p); return &p; }
    T& operator[](size_t i) const { return p[i]; }
    void alloc(size_t count, const char* where) {   // a pinned block of `count` T (at least one); a failure throws and holds nothing
        reset();
        void* q = nullptr;
        check(fgpu_host_alloc(ctx, (count ? count : 1) * sizeof(T), &q), where);
        p = (T*)q;
    }
};

}  // namespace falkor
