// gather_split_bw.hip — sibling of gather_bw.hip for the split-plane row screen: every wave reads random 1 536-B rows
// (the upper 16 bits of a 768-d f32 row: one 16-byte and one 8-byte load per lane, twelve whole 128-B lines) from a 15 GB plane, R rows
// in flight, and then — for PCT % of the rows, decided from the loaded data, so the second read depends on the first — the matching
// 1 536-B row of a second plane.  Next to it the whole 3 072-B row gather the f32 traversal does today, in the same process, and the
// wide form of the screen (gather_wide_kernel: H hi rows in flight, then the survivors again as whole rows, at most R at a time).
//   hipcc -O3 --offload-arch=gfx950 gather_split_bw.hip -o gather_split_bw.bin && ./gather_split_bw.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31);
}

// PCT < 0: whole 3 072-B rows from `hi` (three 16-byte loads per lane), no second read.
template <int R, int PCT>
__global__ void __launch_bounds__(256) gather_split_kernel(const char *__restrict__ hi, const char *__restrict__ lo, uint64_t n_rows, uint32_t iters,
                                                           uint32_t *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint32_t acc = 0;
    for (uint32_t it = 0; it < iters; it++) {
        uint64_t row[R];
#pragma unroll
        for (int r = 0; r < R; r++) row[r] = mix64(wid * 0x100000001b3ull + (uint64_t)it * R + r) % n_rows;
        if (PCT < 0) {
            uint4 v[R][3];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int t = 0; t < 3; t++) v[r][t] = *reinterpret_cast<const uint4 *>(hi + row[r] * 3072 + t * 1024 + lane * 16);
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int t = 0; t < 3; t++) acc += v[r][t].x + v[r][t].y + v[r][t].z + v[r][t].w;
        } else {
            uint4 a[R];
            uint2 b[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                a[r] = *reinterpret_cast<const uint4 *>(hi + row[r] * 1536 + lane * 16);
                b[r] = *reinterpret_cast<const uint2 *>(hi + row[r] * 1536 + 1024 + lane * 8);
            }
            bool need[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t s = a[r].x + a[r].y + a[r].z + a[r].w + b[r].x + b[r].y;
                acc += s;
                // wave-uniform, and a function of the loaded data (the plane holds a constant, so the share is exactly PCT %)
                const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
                need[r] = (mix64(row[r] ^ 0x5bd1e995u) + (s0 == 0x0badf00du)) % 100u < (uint32_t)PCT;
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                a[r] = make_uint4(0u, 0u, 0u, 0u);
                b[r] = make_uint2(0u, 0u);
                if (need[r]) {
                    a[r] = *reinterpret_cast<const uint4 *>(lo + row[r] * 1536 + lane * 16);
                    b[r] = *reinterpret_cast<const uint2 *>(lo + row[r] * 1536 + 1024 + lane * 8);
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) acc += a[r].x + a[r].y + a[r].z + a[r].w + b[r].x + b[r].y;
        }
    }
    if (acc == 123456u) sink[0] = acc;
}

// The wide form of the screen's phase C (search.cuh, wave_screen_hi_rows + wave_dist_rows_planes): H hi rows in flight, then — for PCT %
// of them, decided from the loaded data — the WHOLE row again, hi and lo together, in groups of at most R taken off a wave-uniform mask.
// The hi lines of a survivor are read twice; the second read should find them in the caches.
template <int H, int R, int PCT>
__global__ void __launch_bounds__(256) gather_wide_kernel(const char *__restrict__ hi, const char *__restrict__ lo, uint64_t n_rows, uint32_t iters,
                                                          uint32_t *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint32_t acc = 0;
    for (uint32_t it = 0; it < iters; it++) {
        const uint64_t base = wid * 0x100000001b3ull + (uint64_t)it * H;
        uint4 a[H];
        uint2 b[H];
#pragma unroll
        for (int r = 0; r < H; r++) {
            const uint64_t row = mix64(base + r) % n_rows;
            a[r] = *reinterpret_cast<const uint4 *>(hi + row * 1536 + lane * 16);
            b[r] = *reinterpret_cast<const uint2 *>(hi + row * 1536 + 1024 + lane * 8);
        }
        uint32_t surv = 0;
#pragma unroll
        for (int r = 0; r < H; r++) {
            const uint32_t s = a[r].x + a[r].y + a[r].z + a[r].w + b[r].x + b[r].y;
            acc += s;
            const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
            const uint64_t row = mix64(base + r) % n_rows;
            if ((mix64(row ^ 0x5bd1e995u) + (s0 == 0x0badf00du)) % 100u < (uint32_t)PCT) surv |= 1u << r;
        }
        surv = (uint32_t)__builtin_amdgcn_readfirstlane((int)surv);
        while (surv) {
            uint4 c[R], e[R];
            uint2 d[R], f[R];
            uint32_t m = surv;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (m) {
                    const uint64_t row = mix64(base + (uint32_t)__builtin_ctz(m)) % n_rows;
                    m &= m - 1u;
                    c[r] = *reinterpret_cast<const uint4 *>(hi + row * 1536 + lane * 16);
                    d[r] = *reinterpret_cast<const uint2 *>(hi + row * 1536 + 1024 + lane * 8);
                    e[r] = *reinterpret_cast<const uint4 *>(lo + row * 1536 + lane * 16);
                    f[r] = *reinterpret_cast<const uint2 *>(lo + row * 1536 + 1024 + lane * 8);
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (surv) {
                    surv &= surv - 1u;
                    acc += c[r].x + c[r].y + c[r].z + c[r].w + d[r].x + d[r].y + e[r].x + e[r].y + e[r].z + e[r].w + f[r].x + f[r].y;
                }
            }
        }
    }
    if (acc == 123456u) sink[0] = acc;
}

template <int H, int R, int PCT>
static int run_wide(const char *name, const char *hi, const char *lo, uint64_t n_rows, int wg_per_cu, uint32_t *sink) {
    const uint32_t iters = 400 * 4 / H + 1; // about as many rows per wave as run<4, PCT>
    const int grid = 256 * wg_per_cu;
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    hipLaunchKernelGGL((gather_wide_kernel<H, R, PCT>), dim3(grid), dim3(256), 0, 0, hi, lo, n_rows, 20u, sink);
    CHECK(hipEventRecord(a));
    hipLaunchKernelGGL((gather_wide_kernel<H, R, PCT>), dim3(grid), dim3(256), 0, 0, hi, lo, n_rows, iters, sink);
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, a, b));
    const double rows = (double)grid * 4 * iters * H;
    const double requested = 1536.0 * (1.0 + 2.0 * PCT / 100.0), fresh = 1536.0 * (1.0 + PCT / 100.0); // fresh: without the second hi read
    printf("%-40s H=%d R=%d WG/CU=%d: %7.1f Mrows/s  %7.1f B/row requested (%6.2f TB/s), %7.1f B/row not read before (%6.2f TB/s)\n", name, H, R,
           wg_per_cu, rows / ms / 1e3, requested, rows * requested / ms / 1e9, fresh, rows * fresh / ms / 1e9);
    CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
    return 0;
}

template <int R, int PCT>
static int run(const char *name, const char *hi, const char *lo, uint64_t n_rows, int wg_per_cu, uint32_t *sink) {
    const uint32_t iters = 400;
    const int grid = 256 * wg_per_cu;
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    hipLaunchKernelGGL((gather_split_kernel<R, PCT>), dim3(grid), dim3(256), 0, 0, hi, lo, n_rows, 20u, sink);
    CHECK(hipEventRecord(a));
    hipLaunchKernelGGL((gather_split_kernel<R, PCT>), dim3(grid), dim3(256), 0, 0, hi, lo, n_rows, iters, sink);
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, a, b));
    const double rows = (double)grid * 4 * iters * R;
    const double bytes_per_row = PCT < 0 ? 3072.0 : 1536.0 * (1.0 + PCT / 100.0);
    printf("%-40s R=%d WG/CU=%d: %7.1f Mrows/s  %7.1f B/row  %6.2f TB/s\n", name, R, wg_per_cu, rows / ms / 1e3, bytes_per_row,
           rows * bytes_per_row / ms / 1e9);
    CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
    return 0;
}

int main() {
    const uint64_t n = 10000000; // 10M rows: each plane 15.36 GB, the pair the 30.7 GB of the f32 rows
    char *hi = nullptr, *lo = nullptr;
    uint32_t *sink = nullptr;
    CHECK(hipMalloc((void **)&hi, 2 * n * 1536));
    lo = hi + n * 1536;
    CHECK(hipMalloc((void **)&sink, 16));
    CHECK(hipMemset(hi, 1, 2 * n * 1536));
    for (int wg : {2, 4, 6, 8}) {
        if (run<4, -1>("f32 rows 3 072 B (today)", hi, lo, n, wg, sink)) return 1;
        if (run<4, 0>("hi plane 1 536 B only", hi, lo, n, wg, sink)) return 1;
        if (run<8, 0>("hi plane 1 536 B only", hi, lo, n, wg, sink)) return 1;
        if (run<4, 23>("hi 1 536 B + dependent lo for 23 %", hi, lo, n, wg, sink)) return 1;
        if (run<8, 23>("hi 1 536 B + dependent lo for 23 %", hi, lo, n, wg, sink)) return 1;
        if (run<4, 100>("hi 1 536 B + dependent lo for 100 %", hi, lo, n, wg, sink)) return 1;
        // the wide form next to the shape it replaces, at the two survivor shares seen on the 768-d workloads
        if (run<4, 18>("hi 1 536 B + dependent lo for 18 %", hi, lo, n, wg, sink)) return 1;
        if (run_wide<6, 4, 18>("hi x H, then whole rows for 18 %", hi, lo, n, wg, sink)) return 1;
        if (run_wide<7, 4, 18>("hi x H, then whole rows for 18 %", hi, lo, n, wg, sink)) return 1;
        if (run_wide<7, 4, 23>("hi x H, then whole rows for 23 %", hi, lo, n, wg, sink)) return 1;
    }
    return 0;
}
