// device_mem_selftest — the owning buffer type and the scratch-pool lease of the host side (csrc/device_mem.h) on the CPU, under
// AddressSanitizer + UBSan: no GPU, no library.  The functions the header declares (allocation, scratch pool, pinned host blocks) are defined HERE,
// over malloc / free with counters and a "fail the next N allocations" switch; that link-time seam is the whole hook.  A double free, a leak or a use after free is the
// sanitizer's to report; the counters check what was asked for and in which order.
#include "../csrc/device_mem.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string_view>
#include <utility>

static long g_live = 0, g_allocs = 0, g_frees = 0;
static long g_live_at_last_alloc = -1; // blocks alive at the moment of the most recent request
static size_t g_last_bytes = 0;
static int g_fail_next = 0;
static char g_err[256] = "";

extern "C" void leann_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
void *leann_internal_device_alloc(size_t bytes) {
    g_live_at_last_alloc = g_live;
    g_last_bytes = bytes;
    if (g_fail_next > 0) { g_fail_next--; return nullptr; }
    void *p = malloc(bytes);
    if (p) { g_live++; g_allocs++; }
    return p;
}
void leann_internal_device_release(void *p) {
    if (!p) return;
    g_live--;
    g_frees++;
    free(p);
}
static long g_leased = 0, g_acquires = 0, g_returns = 0; // the "pool": every block is a malloc, handed out and taken back once
static size_t g_last_lease_bytes = 0;
int leann_internal_scratch_acquire(void **out, size_t bytes) {
    *out = nullptr;
    g_last_lease_bytes = bytes;
    if (g_fail_next > 0) { g_fail_next--; leann_set_error("pool: %zu bytes failed", bytes); return LEANN_ERR_DEVICE; }
    *out = malloc(bytes ? bytes : 1);
    g_leased++;
    g_acquires++;
    return LEANN_OK;
}
void leann_internal_scratch_release(void *p) {
    if (!p) return;
    g_leased--;
    g_returns++;
    free(p);
}

static long g_pinned = 0, g_pins = 0, g_unpins = 0; // PinnedBuf's two functions: the "device address" is the host's plus a constant
static size_t g_last_pin_bytes = 0;
void *leann_internal_pinned_alloc(size_t bytes, void **dev) {
    *dev = nullptr;
    g_last_pin_bytes = bytes;
    if (g_fail_next > 0) { g_fail_next--; return nullptr; }
    char *p = static_cast<char *>(malloc(bytes));
    if (p) { g_pinned++; g_pins++; *dev = p + 1; }
    return p;
}
void leann_internal_pinned_release(void *p) {
    if (!p) return;
    g_pinned--;
    g_unpins++;
    free(p);
}

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static void takes_pointers(float *a, const float *b) { CHECK(a == b); }

int main() {
    { // destruction frees exactly once; the conversion hands out the pointer
        DeviceBuf<float> b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.alloc(100) == LEANN_OK);
        CHECK(b.p && b.cap == 100 && g_last_bytes == 400 && g_live == 1);
        takes_pointers(b, b);
        b.p[99] = 1.0f; // the block really has 100 elements (AddressSanitizer)
    }
    CHECK(g_live == 0 && g_allocs == 1 && g_frees == 1);

    { // move: the source is empty, the moved-to buffer frees
        DeviceBuf<float> a;
        CHECK(a.alloc(8) == LEANN_OK);
        float *p = a.p;
        DeviceBuf<float> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 8 && g_live == 1);
        DeviceBuf<float> c;
        CHECK(c.alloc(4) == LEANN_OK && g_live == 2);
        c = std::move(b); // the assigned-to buffer's own block goes first
        CHECK(b.p == nullptr && b.cap == 0 && c.p == p && c.cap == 8 && g_live == 1);
    }
    CHECK(g_live == 0 && g_allocs == g_frees);

    { // grow at or below the capacity: no request, same pointer; above it: the old block is gone when the new one is asked for
        DeviceBuf<unsigned long long> b;
        CHECK(b.grow(10) == LEANN_OK && b.cap == 10 && g_last_bytes == 80);
        unsigned long long *p = b.p;
        const long allocs = g_allocs;
        CHECK(b.grow(10) == LEANN_OK && b.grow(3) == LEANN_OK && b.grow(0) == LEANN_OK);
        CHECK(b.p == p && b.cap == 10 && g_allocs == allocs);
        CHECK(b.grow(11) == LEANN_OK);
        CHECK(g_live_at_last_alloc == 0 && g_allocs == allocs + 1 && b.cap == 11 && g_live == 1);
        b.p[10] = 1;
        b.reset();
        CHECK(b.p == nullptr && b.cap == 0 && g_live == 0);
        b.reset(); // empty: nothing to free
        CHECK(g_allocs == g_frees);
    }

    { // a failed alloc / grow leaves {nullptr, 0} and LEANN_ERR_DEVICE with the byte count in the message; a later grow succeeds
        DeviceBuf<float> b;
        g_fail_next = 1;
        g_err[0] = 0;
        CHECK(b.alloc(1000) == LEANN_ERR_DEVICE && b.p == nullptr && b.cap == 0 && g_live == 0);
        CHECK(std::string_view(g_err).find("4000") != std::string_view::npos);
        CHECK(b.grow(5) == LEANN_OK && b.cap == 5);
        g_fail_next = 1;
        g_err[0] = 0;
        CHECK(b.grow(6) == LEANN_ERR_DEVICE && b.p == nullptr && b.cap == 0 && g_live == 0); // the old block was freed first
        CHECK(std::string_view(g_err).find("24") != std::string_view::npos);
        CHECK(b.grow(2) == LEANN_OK && b.p && b.cap == 2 && g_live == 1);
    }
    CHECK(g_live == 0);

    { // a zero-size request yields a small non-null block, once
        DeviceBuf<float> b;
        CHECK(b.alloc(0) == LEANN_OK && b.p && b.cap == 0 && g_last_bytes > 0 && g_live == 1);
        const long allocs = g_allocs;
        CHECK(b.grow(0) == LEANN_OK && g_allocs == allocs);
        DeviceBuf<float> c;
        CHECK(c.grow(0) == LEANN_OK && c.p && g_live == 2);
    }
    CHECK(g_live == 0);

    { // release: the buffer is empty and the block is the caller's
        float *p = nullptr;
        {
            DeviceBuf<float> b;
            CHECK(b.alloc(16) == LEANN_OK);
            p = b.release();
            CHECK(p && b.p == nullptr && b.cap == 0);
        }
        CHECK(g_live == 1);
        p[15] = 2.0f;
        leann_internal_device_release(p);
        CHECK(g_live == 0);
    }

    { // per-stream scratch: a map entry made by operator[] and grown twice holds one block, none after clear()
        std::map<int, DeviceBuf<float>> m;
        CHECK(m[7].grow(10) == LEANN_OK);
        CHECK(m[7].grow(500) == LEANN_OK);
        CHECK(m.size() == 1 && m[7].cap == 500 && g_live == 1);
        m.clear();
        CHECK(g_live == 0);
    }

    { // converting move: the same block under another element type, the capacity rescaled, the source empty, freed once
        DeviceBuf<float> f;
        CHECK(f.alloc(10) == LEANN_OK);
        void *p = f.p;
        const long frees = g_frees;
        DeviceBuf<unsigned char> bytes(std::move(f));
        CHECK(f.p == nullptr && f.cap == 0 && bytes.p == p && bytes.cap == 40 && g_live == 1 && g_frees == frees);
        bytes.p[39] = 1;
        DeviceBuf<unsigned char> member; // ... and into a member that already exists (a handle adopting a local's rows)
        DeviceBuf<float> g;
        CHECK(g.alloc(3) == LEANN_OK && g_live == 2);
        member = DeviceBuf<unsigned char>(std::move(g));
        CHECK(g.p == nullptr && member.cap == 12 && g_live == 2);
        DeviceBuf<unsigned short> halves(std::move(member)); // 12 bytes -> 6 elements
        CHECK(member.p == nullptr && halves.cap == 6 && g_live == 2);
    }
    CHECK(g_live == 0 && g_allocs == g_frees);

    { // lease: acquire asks the pool for count * sizeof(T) bytes; destruction gives the block back exactly once
        ScratchLease<unsigned long long> a;
        CHECK(a.p == nullptr);
        CHECK(a.acquire(5) == LEANN_OK && a.p && g_last_lease_bytes == 40 && g_leased == 1);
        a.p[4] = 1;
        unsigned long long *q = a;
        CHECK(q == a.p);
    }
    CHECK(g_leased == 0 && g_acquires == 1 && g_returns == 1);

    { // lease moves: the source is empty; an assigned-to lease gives its own block back first; reset() twice returns once
        ScratchLease<float> a, c;
        CHECK(a.acquire(8) == LEANN_OK && c.acquire(2) == LEANN_OK && g_leased == 2);
        float *p = a.p;
        ScratchLease<float> b(std::move(a));
        CHECK(a.p == nullptr && b.p == p && g_leased == 2);
        c = std::move(b);
        CHECK(b.p == nullptr && c.p == p && g_leased == 1);
        const long returns = g_returns;
        c.reset();
        c.reset();
        CHECK(c.p == nullptr && g_leased == 0 && g_returns == returns + 1);
    }

    { // a failed acquire leaves the lease empty and hands the pool's error code on; a later acquire succeeds
        ScratchLease<float> a;
        g_fail_next = 1;
        CHECK(a.acquire(100) == LEANN_ERR_DEVICE && a.p == nullptr && g_leased == 0);
        CHECK(a.acquire(1) == LEANN_OK && a.p && g_leased == 1);
    }
    CHECK(g_leased == 0 && g_acquires == g_returns);

    { // pinned host block: count * sizeof(T) bytes asked for, both addresses kept, freed exactly once; reset() twice frees once; a
      // failed allocation leaves the buffer empty with LEANN_ERR_DEVICE and a later one succeeds; a zero count still yields a block
        PinnedBuf<float> a;
        CHECK(a.p == nullptr && a.dev == nullptr && a.cap == 0);
        CHECK(a.alloc(6) == LEANN_OK && a.p && g_last_pin_bytes == 24 && a.cap == 6 && g_pinned == 1);
        CHECK(reinterpret_cast<char *>(a.dev) == reinterpret_cast<char *>(a.p) + 1);
        a.p[5] = 1.0f;
        const long unpins = g_unpins;
        a.reset();
        a.reset();
        CHECK(a.p == nullptr && a.dev == nullptr && a.cap == 0 && g_pinned == 0 && g_unpins == unpins + 1);
        g_fail_next = 1;
        CHECK(a.alloc(100) == LEANN_ERR_DEVICE && a.p == nullptr && a.dev == nullptr && a.cap == 0 && g_pinned == 0);
        CHECK(a.alloc(0) == LEANN_OK && a.p && a.cap == 0 && g_last_pin_bytes > 0 && g_pinned == 1);
    }
    CHECK(g_pinned == 0 && g_pins == g_unpins && g_pins == 2);

    CHECK(g_live == 0 && g_allocs == g_frees);
    if (g_failed) { fprintf(stderr, "device_mem_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("device_mem_selftest ok: %ld blocks allocated and freed, %ld leases taken and given back\n", g_allocs, g_acquires);
    return 0;
}
