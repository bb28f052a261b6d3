// device_mem.h — who owns device memory.  DeviceBuf<T> is the one owning type of the host side: a scoped temporary, a
// grow-and-keep scratch buffer and a handle's member (internal.h: GraphStore, leann_backend) are the same thing, a pointer that is
// freed exactly once.  ScratchLease<T> is the same for a block of scan.hip's scratch pool: it goes back to the pool exactly once.
// Plain C++17, no HIP types: every allocation goes through the four functions below (defined once, in api.hip over hipMalloc /
// hipFree and in scan.hip over the pool), and the CPU selftest (host/device_mem_selftest.cpp) defines them over malloc / free to
// count what the two types ask for.  PinnedBuf<T> is the host-memory counterpart (two functions of its own, refine.hip).
#pragma once
#include "../../include/leann_backend.h"
#include <cassert>
#include <cstddef>

extern "C" void leann_set_error(const char *fmt, ...);
void *leann_internal_device_alloc(size_t bytes); // on the current device; null on failure
void leann_internal_device_release(void *p);     // null is fine; synchronises the device, as hipFree does
int leann_internal_scratch_acquire(void **out, size_t bytes); // scan.hip's pool, on the current device: blocks are kept for reuse
void leann_internal_scratch_release(void *p);    // null is fine; called by ScratchLease only

template <typename T>
struct DeviceBuf {
    T *p = nullptr;
    size_t cap = 0; // in elements, everywhere

    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    // converting move: the same block seen as another element type (a handle keeps f32, bf16 and feature rows in one byte buffer)
    template <typename U>
    explicit DeviceBuf(DeviceBuf<U> &&o) noexcept : p(reinterpret_cast<T *>(o.p)), cap(o.cap * sizeof(U) / sizeof(T)) { o.p = nullptr; o.cap = 0; }
    ~DeviceBuf() { reset(); }
    operator T *() const { return p; } // kernel arguments and SearchArgs fields take the buffer as they took the pointer

    // `count` elements into an empty buffer (a zero count still yields a small block: callers pass the pointer on unconditionally)
    int alloc(size_t count) {
        assert(!p);
        const size_t bytes = count * sizeof(T);
        p = static_cast<T *>(leann_internal_device_alloc(bytes ? bytes : 16));
        if (!p) { leann_set_error("device allocation of %zu bytes failed", bytes); return LEANN_ERR_DEVICE; }
        cap = count;
        return LEANN_OK;
    }
    // At least `count` elements; the contents are NOT kept.  The old block is freed before the new one is asked for: the peak stays at
    // one block, and the free's device synchronisation means nothing still reads the old one.
    int grow(size_t count) {
        if (p && count <= cap) return LEANN_OK;
        reset();
        return alloc(count);
    }
    T *release() { T *q = p; p = nullptr; cap = 0; return q; } // ownership leaves the type (no caller in the library does this today)
    void reset() { leann_internal_device_release(p); p = nullptr; cap = 0; }
};

// DeviceBuf's host counterpart: a block of pinned host memory that is mapped into the current device's address space, so that a
// kernel reads it in place across the bus (refine.hip: exact rows kept on the host).  `dev` is the address kernels use, `p` the
// host's.  The two functions are defined once, in refine.hip, over hipHostMalloc / hipHostFree; a block counts in
// leann_debug_device_blocks like any other the library owns.
void *leann_internal_pinned_alloc(size_t bytes, void **dev); // null on failure
void leann_internal_pinned_release(void *p);                 // null is fine
template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    T *dev = nullptr;
    size_t cap = 0; // in elements

    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { reset(); }

    int alloc(size_t count) { // into an empty buffer; the caller words the message of a failure
        assert(!p);
        const size_t bytes = count * sizeof(T);
        void *d = nullptr;
        p = static_cast<T *>(leann_internal_pinned_alloc(bytes ? bytes : 16, &d));
        if (!p) return LEANN_ERR_DEVICE;
        dev = static_cast<T *>(d);
        cap = count;
        return LEANN_OK;
    }
    void reset() { leann_internal_pinned_release(p); p = dev = nullptr; cap = 0; }
};

// A block of the scratch pool, given back by the destructor.  The pool's rule is the holder's to keep: every stream that touched the
// block has been synchronised by the time the lease ends.
template <typename T>
struct ScratchLease {
    T *p = nullptr;

    ScratchLease() = default;
    ScratchLease(const ScratchLease &) = delete;
    ScratchLease &operator=(const ScratchLease &) = delete;
    ScratchLease(ScratchLease &&o) noexcept : p(o.p) { o.p = nullptr; }
    ScratchLease &operator=(ScratchLease &&o) noexcept {
        if (this != &o) { reset(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~ScratchLease() { reset(); }
    operator T *() const { return p; }

    int acquire(size_t count) { // into an empty lease; a failure (the pool has set the error) leaves it empty
        assert(!p);
        void *q = nullptr;
        const int rc = leann_internal_scratch_acquire(&q, count * sizeof(T));
        p = rc == LEANN_OK ? static_cast<T *>(q) : nullptr;
        return rc;
    }
    void reset() { leann_internal_scratch_release(p); p = nullptr; }
};
