// refine.hip — refining search results on exact f32 rows (include/leann_backend.h "refining results on exact rows").
// A walk over narrow rows (bf16, int8) or over recomputed ones fetches fetch_k candidates; rerank_kernel re-scores them on the exact
// rows with the distance the f32 traversal computes (wave_dist_rows, search.cuh) and returns the best top_k by (dist, key).  The
// exact rows sit in HBM or in pinned host memory the kernel reads in place: 10-40 rows per query are little enough for the bus.
//
//   rerank_kernel<T, R>   one workgroup of four waves per query.  Each wave stages the query as float4 q[T] and takes a contiguous
//                         quarter of the candidates in groups of R rows whose loads are all issued before the first use; lane 0
//                         writes orderable(dist) << 32 | (key - key_offset) into an LDS array padded with ~0 to a power of two,
//                         bitonic_sort_lds orders it, the first top_k entries go out with the key offset added back.
//
// Every key is range-checked before an address is formed from it: a list with garbage in it is skipped entry by entry (and counted),
// it cannot make the kernel read outside the rows.  R per T (refine_R below) is the largest group up to 16 rows that keeps the kernel
// within 256 vector registers without a spill (-Rpass-analysis=kernel-resource-usage; the table is in DESIGN.md §9e), so that two
// workgroups share a CU.  8 KiB of LDS: the sort array alone.
#include "internal.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

#define REFINE_MAX_K 1024 // fetch_k: the sort array holds this many u64 keys (8 KiB)

struct RerankArgs {
    const float *X;       // exact rows [n x ld], device-readable
    uint64_t n;           // rows; < 2^32 - 1, so that no entry equals the padding value
    uint32_t ld, d;
    uint64_t key_offset;
    const float *queries; // [nq x d]
    const uint64_t *keys; // [nq x fetch_k]
    const uint32_t *counts;
    uint32_t fetch_k, top_k;
    uint64_t *out_keys;   // [nq x top_k]
    float *out_dists;
    uint32_t *out_counts, *skipped; // skipped: optional
};

template <int T, int R>
__global__ void __launch_bounds__(256, 2) rerank_kernel(const RerankArgs a) {
    __shared__ uint64_t s_sort[REFINE_MAX_K];
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t m = min(a.counts[q], a.fetch_k);
    uint32_t npow = 1;
    while (npow < m) npow <<= 1;
    for (uint32_t i = m + threadIdx.x; i < npow; i += blockDim.x) s_sort[i] = ~0ull;

    float4 qv[T];
    const float *qrow = a.queries + (size_t)q * a.d;
#pragma unroll
    for (int t = 0; t < T; t++) qv[t] = vec_load4_guard(qrow, a.d, t, lane);

    // this wave's quarter of the list, in groups of R: the valid candidates of a group are packed to the front of ids[] (a chain of
    // selects on wave-uniform values: no register array is indexed by a run-time value), their rows are read together
    const uint64_t *list = a.keys + (size_t)q * a.fetch_k;
    const uint32_t per = (m + 3) / 4, c_end = min(m, (wave + 1) * per);
    for (uint32_t c0 = wave * per; c0 < c_end; c0 += R) {
        uint32_t ids[R] = {}, slot[R] = {};
        int nv = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t c = c0 + r;
            if (c < c_end) {
                const uint64_t key = list[c];
                const uint64_t pos = key - a.key_offset;
                const bool valid = uni(key >= a.key_offset && pos < a.n);
                if (valid) {
                    const uint32_t p = uni((uint32_t)pos);
#pragma unroll
                    for (int j = 0; j <= r; j++)
                        if (nv == j) { ids[j] = p; slot[j] = c; }
                    nv++;
                } else if (lane == 0) {
                    s_sort[c] = ~0ull; // skipped: out of the rows' range (the UINT64_MAX tail value included); no row is read
                }
            }
        }
        float dd[R];
        wave_dist_rows<T, R>(qv, a.X, a.ld, ids, nv, lane, dd);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < nv) s_sort[slot[r]] = ((uint64_t)f32_orderable(dd[r]) << 32) | ids[r];
        }
    }
    bitonic_sort_lds(s_sort, (int)npow); // (starts and ends with a barrier)

    for (uint32_t i = threadIdx.x; i < a.top_k; i += blockDim.x) {
        const uint64_t e = i < npow ? s_sort[i] : ~0ull;
        a.out_keys[(size_t)q * a.top_k + i] = e != ~0ull ? a.key_offset + (uint32_t)e : ~0ull;
        a.out_dists[(size_t)q * a.top_k + i] = e != ~0ull ? orderable_f32((uint32_t)(e >> 32)) : __int_as_float(0x7F800000);
    }
    // the valid entries are the sorted array's prefix in front of the first ~0: exactly one thread sees its end
    for (uint32_t i = threadIdx.x; i < npow; i += blockDim.x) {
        const bool here = s_sort[i] != ~0ull, next = i + 1 < npow && s_sort[i + 1] != ~0ull;
        const uint32_t v = here ? i + 1 : 0;
        if ((here && !next) || (!here && i == 0)) {
            a.out_counts[q] = min(v, a.top_k);
            if (a.skipped) a.skipped[q] = m - v;
        }
    }
}

// rows in flight per wave, by width (chunks of 256 floats)
constexpr int refine_R(int T) { return T <= 3 ? 16 : T == 4 ? 13 : T == 6 ? 8 : T == 8 ? 6 : T == 12 ? 3 : 2; }
using RerankKernel = void (*)(const RerankArgs);
template <int T>
static RerankKernel rerank_for() { return rerank_kernel<T, refine_R(T)>; }
static RerankKernel rerank_kernel_of(int T) {
    switch (T) {
        case 1: return rerank_for<1>();
        case 2: return rerank_for<2>();
        case 3: return rerank_for<3>();
        case 4: return rerank_for<4>();
        case 6: return rerank_for<6>();
        case 8: return rerank_for<8>();
        case 12: return rerank_for<12>();
        case 16: return rerank_for<16>();
        default: return nullptr;
    }
}

// ---- pinned, device-mapped host memory (device_mem.h: PinnedBuf) ---------------------------------------------------------------------
void *leann_internal_pinned_alloc(size_t bytes, void **dev) {
    void *p = nullptr;
    *dev = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipHostGetDevicePointer(dev, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(p);
        return nullptr;
    }
    leann_internal_device_blocks++;
    return p;
}
void leann_internal_pinned_release(void *p) {
    if (!p) return;
    leann_internal_device_blocks--;
    (void)hipHostFree(p);
}

// ---- the rows ------------------------------------------------------------------------------------------------------------------------
struct leann_exact_rows {
    const float *X = nullptr; // what the kernel reads: borrowed rows, `hbm`, or the device address of `host`
    size_t n = 0, dims = 0, ld = 0;
    int device = 0, placement = LEANN_EXACT_ROWS_HBM;
    uint64_t key_offset = 0;
    DeviceBuf<float> hbm;
    PinnedBuf<float> host;
};

static int check_rows_shape(const char *who, size_t n, size_t dims, int placement, const void *out) {
    if (!out) { leann_set_error("%s: null out", who); return LEANN_ERR_INVALID; }
    if (dims < 1 || dims > 4096) { leann_set_error("%s: dims = %zu is outside [1, 4096]", who, dims); return LEANN_ERR_INVALID; }
    if (n >= 0xFFFFFFFFull) { leann_set_error("%s: n = %zu is 2^32 - 1 or more", who, n); return LEANN_ERR_INVALID; }
    if (placement != LEANN_EXACT_ROWS_HBM && placement != LEANN_EXACT_ROWS_HOST) {
        leann_set_error("%s: placement = %d is neither 0 (LEANN_EXACT_ROWS_HBM) nor 1 (LEANN_EXACT_ROWS_HOST)", who, placement);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
static int select_device(int device) {
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    return LEANN_OK;
}
static int pinned_rows(const char *who, leann_exact_rows *r) {
    if (r->host.alloc(std::max<size_t>(r->n * r->ld, 4))) {
        leann_set_error("%s: %zu bytes of pinned, device-mapped host memory for the exact rows could not be had; placement 0 "
                        "(LEANN_EXACT_ROWS_HBM) keeps them in device memory instead", who, r->n * r->ld * 4);
        return LEANN_ERR_DEVICE;
    }
    r->X = r->host.dev;
    return LEANN_OK;
}

extern "C" int leann_exact_rows_from_device(const float *d_rows, size_t n, size_t dims, size_t ld, int device, uint64_t key_offset,
                                            leann_exact_rows **out) {
    const char *who = "leann_exact_rows_from_device";
    if (out) *out = nullptr;
    if (int rc = check_rows_shape(who, n, dims, LEANN_EXACT_ROWS_HBM, out)) return rc;
    if (!d_rows) { leann_set_error("%s: null d_rows", who); return LEANN_ERR_INVALID; }
    if (ld < dims || ld % 4 != 0) { leann_set_error("%s: ld = %zu must be a multiple of 4 and at least dims = %zu", who, ld, dims); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    leann_exact_rows *r = new leann_exact_rows();
    r->X = d_rows; r->n = n; r->dims = dims; r->ld = ld; r->device = device; r->key_offset = key_offset;
    *out = r;
    return LEANN_OK;
}

extern "C" int leann_exact_rows_from_host(const float *rows, size_t n, size_t dims, int device, uint64_t key_offset, int placement,
                                          leann_exact_rows **out) {
    const char *who = "leann_exact_rows_from_host";
    if (out) *out = nullptr;
    if (int rc = check_rows_shape(who, n, dims, placement, out)) return rc;
    if (!rows && n) { leann_set_error("%s: null rows", who); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    if (int rc = select_device(device)) return rc;
    std::unique_ptr<leann_exact_rows> r(new leann_exact_rows());
    r->n = n; r->dims = dims; r->ld = (dims + 3) & ~(size_t)3; r->device = device; r->key_offset = key_offset; r->placement = placement;
    if (placement == LEANN_EXACT_ROWS_HOST) {
        if (int rc = pinned_rows(who, r.get())) return rc;
        if (r->ld != dims) memset(r->host.p, 0, std::max<size_t>(n * r->ld, 4) * 4);
        for (size_t i = 0; i < n; i++) memcpy(r->host.p + i * r->ld, rows + i * dims, dims * 4);
    } else {
        if (int rc = r->hbm.alloc(std::max<size_t>(n * r->ld, 4))) return rc;
        if (n && leann_internal_stage_rows(r->hbm, r->ld, rows, dims, dims, n, true) != hipSuccess) {
            leann_set_error("%s: copy of %zu rows to the device failed", who, n);
            return LEANN_ERR_DEVICE;
        }
        r->X = r->hbm;
    }
    *out = r.release();
    return LEANN_OK;
}

extern "C" int leann_exact_rows_open(const char *embeddings_path, size_t dims, int device, uint64_t key_offset, int placement,
                                     leann_exact_rows **out) {
    const char *who = "leann_exact_rows_open";
    if (out) *out = nullptr;
    if (int rc = check_rows_shape(who, 0, dims, placement, out)) return rc;
    if (!embeddings_path) { leann_set_error("%s: null embeddings_path", who); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    struct stat st{};
    if (stat(embeddings_path, &st) != 0) {
        leann_set_error("%s: %s not found (`leann build --recompute` writes the exact rows beside the index)", who, embeddings_path);
        return LEANN_ERR_NOT_FOUND;
    }
    if (st.st_size == 0 || (uint64_t)st.st_size % (dims * 4) != 0) {
        leann_set_error("%s: %lld bytes is not a whole number of %zu-dimensional f32 embeddings", embeddings_path, (long long)st.st_size, dims);
        return LEANN_ERR_FORMAT;
    }
    const size_t n = (size_t)st.st_size / (dims * 4);
    if (n >= 0xFFFFFFFFull) { leann_set_error("%s: too many embeddings (%zu)", embeddings_path, n); return LEANN_ERR_FORMAT; }
    std::unique_ptr<leann_exact_rows> r(new leann_exact_rows());
    r->n = n; r->dims = dims; r->ld = (dims + 3) & ~(size_t)3; r->device = device; r->key_offset = key_offset; r->placement = placement;
    if (placement == LEANN_EXACT_ROWS_HBM) { // the reader of a stock directory's rows (handle.hip)
        const int rc = leann_internal_rows_from_file(embeddings_path, 0, n, dims, device, &r->hbm);
        if (rc == LEANN_ERR_NOT_FOUND) { leann_set_error("cannot open %s", embeddings_path); return LEANN_ERR_IO; }
        if (rc == LEANN_ERR_IO) leann_set_error("reading %s into device memory failed", embeddings_path);
        if (rc) return rc;
        r->X = r->hbm;
    } else { // the same rows, at the same pitch, read straight into the pinned block
        std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(embeddings_path, "rb"), fclose);
        if (!f) { leann_set_error("cannot open %s", embeddings_path); return LEANN_ERR_IO; }
        if (int rc = select_device(device)) return rc;
        if (int rc = pinned_rows(who, r.get())) return rc;
        if (r->ld != dims) memset(r->host.p, 0, n * r->ld * 4);
        const bool ok = r->ld == dims ? fread(r->host.p, dims * 4, n, f.get()) == n : [&] {
            for (size_t i = 0; i < n; i++)
                if (fread(r->host.p + i * r->ld, 4, dims, f.get()) != dims) return false;
            return true;
        }();
        if (!ok) { leann_set_error("reading %s into pinned host memory failed", embeddings_path); return LEANN_ERR_IO; }
    }
    *out = r.release();
    return LEANN_OK;
}

extern "C" size_t leann_exact_rows_len(const leann_exact_rows *r) { return r ? r->n : 0; }
extern "C" int leann_exact_rows_placement(const leann_exact_rows *r) { return r ? r->placement : -1; }
extern "C" void leann_exact_rows_close(leann_exact_rows *r) {
    if (!r) return;
    if (r->hbm.p || r->host.p) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize(); // no kernel still reads the rows
    }
    delete r;
}

// ---- the rerank ----------------------------------------------------------------------------------------------------------------------
static int check_k(const char *who, size_t top_k, size_t fetch_k) {
    if (top_k < 1) { leann_set_error("%s: top_k = 0", who); return LEANN_ERR_INVALID; }
    if (fetch_k > REFINE_MAX_K) { leann_set_error("%s: fetch_k = %zu is above %d", who, fetch_k, REFINE_MAX_K); return LEANN_ERR_INVALID; }
    if (top_k > fetch_k) { leann_set_error("%s: top_k = %zu is above fetch_k = %zu", who, top_k, fetch_k); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}

extern "C" int leann_rerank_batch_device(const leann_exact_rows *r, const float *d_queries, size_t nq, const uint64_t *d_keys,
                                         const uint32_t *d_counts, size_t fetch_k, size_t top_k, uint64_t *d_out_keys, float *d_out_dists,
                                         uint32_t *d_out_counts, uint32_t *d_skipped, void *stream) {
    const char *who = "leann_rerank_batch_device";
    if (!r) { leann_set_error("%s: null rows", who); return LEANN_ERR_INVALID; }
    if (nq && (!d_queries || !d_keys || !d_counts || !d_out_keys || !d_out_dists || !d_out_counts)) {
        leann_set_error("%s: null %s", who, !d_queries ? "d_queries" : !d_keys ? "d_keys" : !d_counts ? "d_counts" : !d_out_keys ? "d_out_keys"
                                            : !d_out_dists ? "d_out_dists" : "d_out_counts");
        return LEANN_ERR_INVALID;
    }
    if (int rc = check_k(who, top_k, fetch_k)) return rc;
    if (nq >= (1ull << 31)) { leann_set_error("%s: nq = %zu is 2^31 or more", who, nq); return LEANN_ERR_INVALID; }
    RerankKernel kernel = rerank_kernel_of(search_width_T((uint32_t)((r->ld + 255) / 256)));
    if (!kernel) { leann_set_error("%s: no kernel for rows of %zu floats", who, r->ld); return LEANN_ERR_INVALID; }
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(r->device));
    RerankArgs a{};
    a.X = r->X; a.n = r->n; a.ld = (uint32_t)r->ld; a.d = (uint32_t)r->dims; a.key_offset = r->key_offset;
    a.queries = d_queries; a.keys = d_keys; a.counts = d_counts; a.fetch_k = (uint32_t)fetch_k; a.top_k = (uint32_t)top_k;
    a.out_keys = d_out_keys; a.out_dists = d_out_dists; a.out_counts = d_out_counts; a.skipped = d_skipped;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)nq), dim3(256), 0, (hipStream_t)stream, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

// ---- walk, then rerank ---------------------------------------------------------------------------------------------------------------
static int refined_check(const char *who, const leann_backend *h, const leann_exact_rows *r, const void *queries, size_t nq, size_t top_k,
                         size_t fetch_k, const void *keys, const void *dists, const void *counts) {
    if (!h || !r || (nq && (!queries || !keys || !dists || !counts))) {
        leann_set_error("%s: null %s", who, !h ? "handle" : !r ? "rows" : !queries ? "queries" : !keys ? "keys" : !dists ? "dists" : "counts");
        return LEANN_ERR_INVALID;
    }
    if (int rc = check_k(who, top_k, fetch_k)) return rc;
    if (r->dims != h->g.d) {
        leann_set_error("%s: the rows have dims = %zu, the index %u", who, r->dims, h->g.d);
        return LEANN_ERR_INVALID;
    }
    if (r->device != h->device) {
        leann_set_error("%s: the rows are on device %d, the index on device %d", who, r->device, h->device);
        return LEANN_ERR_INVALID;
    }
    const uint64_t lo = h->sharded ? leann_internal_sharded_lo(h->sharded, 0) : h->key_offset;
    if (r->key_offset > lo || lo + h->g.n > r->key_offset + r->n) {
        leann_set_error("%s: the rows cover positions [%llu, %llu), the index needs key_offset .. key_offset + len = [%llu, %llu)", who,
                        (unsigned long long)r->key_offset, (unsigned long long)(r->key_offset + r->n), (unsigned long long)lo,
                        (unsigned long long)(lo + h->g.n));
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
static int refined_run(const char *who, const leann_backend *h, const leann_exact_rows *r, const float *d_queries, size_t nq, size_t top_k,
                       size_t fetch_k, size_t complexity, const uint8_t *d_allow, size_t allow_stride, uint64_t *d_keys, float *d_dists,
                       uint32_t *d_counts, uint32_t *d_stats, hipStream_t st) {
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    // the walk's lists: {keys | dists | counts} of one lease
    const size_t o_dists = nq * fetch_k * 8, o_counts = o_dists + ((nq * fetch_k * 4 + 7) & ~(size_t)7);
    ScratchLease<unsigned char> lists;
    if (int rc = lists.acquire(o_counts + nq * 4)) return rc;
    uint64_t *w_keys = reinterpret_cast<uint64_t *>(lists.p);
    float *w_dists = reinterpret_cast<float *>(lists.p + o_dists);
    uint32_t *w_counts = reinterpret_cast<uint32_t *>(lists.p + o_counts);
    int rc = leann_backend_search_filtered_batch_device(h, d_queries, nq, fetch_k, complexity, d_allow, allow_stride, w_keys, w_dists,
                                                        w_counts, d_stats, st);
    if (rc == LEANN_OK) rc = leann_rerank_batch_device(r, d_queries, nq, w_keys, w_counts, fetch_k, top_k, d_keys, d_dists, d_counts, nullptr, st);
    // the lease ends with the call: nothing may still be reading the lists
    if (hipStreamSynchronize(st) != hipSuccess && rc == LEANN_OK) {
        leann_set_error("%s: the walk or the rerank failed on the device", who);
        rc = LEANN_ERR_DEVICE;
    }
    return rc;
}

extern "C" int leann_backend_search_refined_batch_device(const leann_backend *h, const leann_exact_rows *r, const float *d_queries, size_t nq,
                                                         size_t top_k, size_t fetch_k, size_t complexity, const uint8_t *d_allow,
                                                         size_t allow_stride, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                                         uint32_t *d_stats, void *stream) {
    const char *who = "leann_backend_search_refined_batch_device";
    if (int rc = refined_check(who, h, r, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    return refined_run(who, h, r, d_queries, nq, top_k, fetch_k, complexity, d_allow, allow_stride, d_keys, d_dists, d_counts, d_stats,
                       (hipStream_t)stream);
}

extern "C" int leann_backend_search_refined_batch(const leann_backend *h, const leann_exact_rows *r, const float *queries, size_t nq,
                                                  size_t top_k, size_t fetch_k, size_t complexity, const uint8_t *allow, size_t allow_stride,
                                                  uint64_t *keys, float *dists, uint32_t *counts, uint32_t *stats) {
    const char *who = "leann_backend_search_refined_batch";
    if (int rc = refined_check(who, h, r, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    if (!allow && allow_stride) { leann_set_error("%s: allow_stride = %zu without an allow-bitmap", who, allow_stride); return LEANN_ERR_INVALID; }
    if (allow && allow_stride && allow_stride < (h->g.n + 7) / 8) {
        leann_set_error("%s: allow_stride = %zu is below ceil(len / 8) = %zu", who, allow_stride, (size_t)(h->g.n + 7) / 8);
        return LEANN_ERR_INVALID;
    }
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    const size_t d = h->g.d;
    DeviceBuf<float> d_q, d_dists;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts, d_stats;
    DeviceBuf<uint8_t> d_allow;
    if (int rc = d_q.alloc(nq * d)) return rc;
    if (int rc = d_keys.alloc(nq * top_k)) return rc;
    if (int rc = d_dists.alloc(nq * top_k)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    if (int rc = d_stats.alloc(nq * 4)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * d * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemset(d_stats, 0, nq * 16));
    if (allow) {
        const size_t total = allow_stride ? allow_stride * nq : (h->g.n + 7) / 8;
        if (int rc = d_allow.alloc(total)) return rc;
        HIP_CHECK_RET(hipMemcpy(d_allow, allow, total, hipMemcpyHostToDevice));
    }
    if (int rc = refined_run(who, h, r, d_q, nq, top_k, fetch_k, complexity, allow ? d_allow.p : nullptr, allow_stride, d_keys, d_dists, d_counts,
                             d_stats, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    if (stats) HIP_CHECK_RET(hipMemcpy(stats, d_stats, nq * 16, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
