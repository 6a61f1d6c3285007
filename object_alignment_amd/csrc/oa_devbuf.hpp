// oa_devbuf.hpp -- DevBuf<T>, the one owner of a block of device memory: a T* that releases its block when it is reset,
// allocated again, assigned over or destroyed.  Plain host C++, no HIP type: tests/c/devbuf_lifetime.cpp checks
// these rules with a host compiler under sanitizers, against a counting allocator.
#pragma once

#include <cstddef>

namespace oa {

// The allocator behind every handle (oa_icp.hip: the process-wide cache).  dev_block_alloc returns the runtime's error code, 0 =
// success.  settled: the device has been synchronised and nothing will touch the block again -- no ordering against a stream.
int dev_block_alloc(void **out, size_t bytes);
void dev_block_release(void *p, bool settled);

// While one lives, this thread's releases are settled: oa_destroy opens it behind its one device synchronisation.
class DevTeardown {
    bool before_;
public:
    static bool &active() { static thread_local bool on = false; return on; }
    DevTeardown() : before_(active()) { active() = true; }
    ~DevTeardown() { active() = before_; }
    DevTeardown(const DevTeardown &) = delete;
    DevTeardown &operator=(const DevTeardown &) = delete;
};

template <typename T> struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    int alloc_bytes(size_t bytes) { reset(); return dev_block_alloc((void **)&p, bytes); }
    int alloc(size_t n) { return alloc_bytes(sizeof(T) * (n ? n : 1)); }
    void reset() { if (p) { dev_block_release((void *)p, DevTeardown::active()); p = nullptr; } }
    operator T *() const { return p; }     // launches, null tests and pointer arithmetic read it as the pointer it holds
    T *operator->() const { return p; }
    template <typename U> explicit operator U *() const { return (U *)p; }   // ... and so does a written cast: (const float *)d_src4
};

}  // namespace oa
