// device_mem.h — who owns device memory.  DeviceBuf<T> is the one owning type of the host side: a scoped temporary, a
// grow-and-keep scratch buffer and a handle's member are the same thing, a pointer that is freed exactly once.  Plain C++17, no HIP
// types: every allocation goes through the two functions below (defined once, in api.hip, over hipMalloc / hipFree), and the CPU
// selftest (host/device_mem_selftest.cpp) defines them over malloc / free to count what this type asks for.
#pragma once
#include "../../include/leann_backend.h"
#include <cassert>
#include <cstddef>

extern "C" void leann_set_error(const char *fmt, ...);
void *leann_internal_device_alloc(size_t bytes); // on the current device; null on failure
void leann_internal_device_release(void *p);     // null is fine; synchronises the device, as hipFree does

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
    T *release() { T *q = p; p = nullptr; cap = 0; return q; } // ownership passes on (to a GraphView field, say)
    void reset() { leann_internal_device_release(p); p = nullptr; cap = 0; }
};
